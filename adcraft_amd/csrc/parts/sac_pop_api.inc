// sac_pop_api.inc - the extern "C" entry points of SAC learner populations: M soft actor-critic learners in lock-step on one engine,
// every launch over all members (include/adcraft_engine.h; the kernels are parts/kernel_sac_pop.inc, the k_td3_pop_* of
// parts/kernel_td3_pop.inc and the k_pg_pop_* of parts/kernel_pg.inc; the law is csrc/adc_sac.h).  The population lives in the TD3
// population's engine fields and shares parts/offpolicy_core.inc with the other front ends (the ring, the critic upload, the state
// vectors, the allocation, tp_params_copy, tp_csum_launch, tp_wgrad_launch, tp_step_run, the update driver): td3_flat / td3_mom
// are [M][P] and [M][2 Qc] (no target actor), the scratch [M][B][...], td3_sums [M][16], tp_cfg what those helpers read of a
// member's configuration (sac_as_td3), the step table three rows per update (critic, actor, temperature).  What TD3 lacks - the
// law's SAC constants, the target entropy, the temperature cell - is in SacMember[M].
// (part of the single translation unit adc_engine.hip)
namespace {
int sp_ready(const adc_engine *e)
{
    if (!e->have_sac_pop)
        return fail(ADC_ESTATE, "adc_engine_sac_pop_init has not been called (or the policy, the learners or the record were re-initialised since)");
    return ADC_OK;
}
// what a SAC population call needs of the engine's state, checked at init and again at every call
int sp_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (e->lrn_M == 0) return fail(ADC_ESTATE, "population training needs learners (adc_engine_mlp_learners)");
    if (e->mp.bd_lo) return fail(ADC_ESTATE, "soft actor-critic training under the bounded act is not supported: it needs a log-probability (adc_engine_mlp_learners_set_bounds(NULL, NULL) first)");
    if (!e->mp.two_heads) return fail(ADC_ESTATE, "SAC needs the two-headed policy (2A outputs: means, log-stds): the free log_std head is not supported");
    if (!e->mp.clamp) return fail(ADC_ESTATE, "SAC needs clamp_log_std on: the log-std head is unbounded without it");
    if (!e->mp.sq_lo) return fail(ADC_ESTATE, "a SAC population needs the learners' squashed action (adc_engine_mlp_learners_set_squash)");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "soft actor-critic training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "soft actor-critic training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
// a member's rows of the two tables from its configuration: the law constants, its key, its target entropy (the cell is state)
void sp_member_fill(adc_engine *e, size_t m, const adc_sac_config &c)
{
    e->tp_mem[m].law = adc::td3_law_of(sac_as_td3(c));         // (k_td3_pop_polyak reads law.tau)
    e->tp_mem[m].key = adc::td3_key(c.seed ? c.seed : e->cfg.seed);
    e->sp_mem[m].law = adc::sac_law_of(e->mlp_cfg, c);
    e->sp_mem[m].target_entropy = c.target_entropy;
}
int sp_members_upload(adc_engine *e)
{
    HIP_TRY(hipMemcpyAsync(e->tp_dmem, e->tp_mem.data(), e->tp_mem.size() * sizeof(Td3Member), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->sp_dmem, e->sp_mem.data(), e->sp_mem.size() * sizeof(SacMember), hipMemcpyHostToDevice, e->stream));
    return ADC_OK;
}
// rows 3 index .. 3 index + 2 of the step table: every member's constants of update `update`'s critic, actor and temperature steps
// (all three count t = update + 1); no clip until a scale is known
void sp_steps_fill(adc_engine *e, int index, int64_t update)
{
    const size_t M = (size_t)e->lrn_M;
    for (size_t m = 0; m < M; ++m) {
        const adc_sac_config &c = e->sp_cfg[m];
        const float lr[3] = {c.critic_lr, c.actor_lr, c.alpha_lr};
        for (size_t k = 0; k < 3; ++k) {
            Td3PopStep &s = e->tp_steps[((size_t)index * 3u + k) * M + m];
            s.clip = 0; s.scale = 1.0f;
            s.step = td3_step_of(e->tp_cfg[m], lr[k], update);
        }
    }
}
// one update of every member; `index`: the update's place in the call's block of kTd3PopBlock (its rows of the step table).
// The members' sums as in the solo path: [0..7] the pieces, [8] the critics' grad^2, [9] the actor's grad^2
int sp_one_update(adc_engine *e, int index, bool stats_wanted, bool last, bool any_clip, bool any_alpha)
{
    const adc::Td3Shape &sh = e->td3_shape;
    const int M = e->lrn_M, B = e->td3_cfg.batch_size, DA = sh.D + sh.A;
    const int nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q), ph = adc::td3_hidden(sh.pol), po = adc::td3_outs(sh.pol);
    const size_t lds = sac_lds_floats(sh) * sizeof(float);
    const dim3 grid((unsigned)B, (unsigned)M);
    SacView p{};
    p.sh = sh;
    p.size = (uint32_t)td3_size(e); p.update = (uint32_t)e->td3_updates;
    p.ybuf = e->td3_ybuf; p.xin = e->td3_xin; p.acts = e->td3_acts; p.deltas = e->td3_deltas; p.pieces = e->td3_pieces;
    p.maxw = adc::td3_max_width(sh);
    sac_norm_fill(e, p);
    td3_per_fill(e, p);
    p.na = 2 * nh; p.nd = 2 * no;
    int rc;
    if (e->per_live && (rc = per_sample_run(e, p.update))) return rc;
    const bool norm = sac_norm_on(p);
    hipLaunchKernelGGL(norm ? k_sac_pop_target<true> : k_sac_pop_target<false>, grid, dim3(kPgBlock), lds, e->stream, p, e->lrn_tab, e->tp_dmem, e->sp_dmem);
    hipLaunchKernelGGL(norm ? k_sac_pop_critic_sample<true> : k_sac_pop_critic_sample<false>, grid, dim3(kPgBlock), lds, e->stream, p, e->tp_dmem);
    for (int i = 0; i < 2; ++i) tp_wgrad_launch(e, sh.q, DA, p.na, i * nh, p.nd, i * no, i * e->td3_Qc, 2 * e->td3_Qc, B);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_leaves_run(e))) return rc;
    if ((rc = tp_step_run(e, kTd3Psi, e->td3_mom + 2, 2 * e->td3_Qc, B, stats_wanted && last, 8, 3 * index, any_clip))) return rc;
    p.na = ph; p.nd = po;
    hipLaunchKernelGGL(norm ? k_sac_pop_actor_sample<true> : k_sac_pop_actor_sample<false>, grid, dim3(kPgBlock), lds, e->stream, p, e->lrn_tab, e->tp_dmem, e->sp_dmem);
    tp_wgrad_launch(e, sh.pol, DA, p.na, 0, p.nd, 0, 0, e->td3_P, B);
    HIP_TRY(hipGetLastError());
    // (the pieces' sums of every update: the temperature's step reads lp's)
    if ((rc = tp_csum_launch(e, e->td3_pieces, B, (size_t)B, adc::kTd3Pieces, adc::kTd3Pieces, 0, 0))) return rc;
    if ((rc = tp_step_run(e, kTd3Theta, e->td3_mom, e->td3_P, B, stats_wanted && last, 9, 3 * index + 1, any_clip))) return rc;
    if (any_alpha)
        hipLaunchKernelGGL(k_sac_pop_alpha, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, e->stream, M, e->sp_dmem, e->td3_sums + adc::kSacLp, 16, (long long)B,
                           e->tp_dsteps + (size_t)(3 * index + 2) * (size_t)M);
    if ((e->td3_updates + 1) % e->sp_cfg[0].target_update_interval == 0) {
        const PgLayout &lay = e->td3_lay[kTd3PsiT];
        hipLaunchKernelGGL(k_td3_pop_polyak, dim3(pg_blocks(lay.Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, lay, e->tp_stride[kTd3PsiT],
                           e->td3_flat[kTd3PsiT], e->td3_flat[kTd3Psi], e->tp_dmem);
    }
    HIP_TRY(hipGetLastError());
    e->td3_updates += 1;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_sac_pop_init(adc_engine *e, const adc_sac_config *cfgs, int32_t count)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sp_state_check(e)) return rc;
    const int N = e->v.N, M = e->lrn_M;
    const char *why = nullptr;
    if (adc_sac_pop_config_check(cfgs, count, N, M, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (e->have_pg || e->have_pg_pop)
        return fail(ADC_ESTATE, "a policy-gradient trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_sac) return fail(ADC_ESTATE, "a single-learner soft actor-critic trainer is alive on this engine (adc_engine_sac_init)");
    if (e->on.live)
        return fail(ADC_ESTATE, "a running observation normaliser is alive on this engine: the replay ring would hold inputs normalised by older vectors");
    const adc::Td3Shape sh = adc::sac_shape_of(e->mlp_cfg, e->v.K, cfgs[0], mlp_frames(e));
    if (sac_lds_floats(sh) * sizeof(float) > 64u * 1024u)
        return fail(ADC_EINVAL, sac_lds_floats(adc::sac_shape_of(e->mlp_cfg, e->v.K, cfgs[0])) * sizeof(float) > 64u * 1024u
                                    ? "num_keywords too large for soft actor-critic training (LDS)"
                                    : "frames: the stacked input row is too large for soft actor-critic training (LDS); fewer frames fit");
    ENGINE_GUARD(e);
    const size_t Ms = (size_t)M, C = (size_t)cfgs[0].capacity;
    const OffBlock k = off_block_layout(sh, 4);
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    OffBufs o;
    float *block = nullptr, *cells = nullptr;
    Td3Member *dmem = nullptr;
    SacMember *smem = nullptr;
    Td3PopStep *dsteps = nullptr;
    int rc;
    if ((rc = off_alloc(e, fresh, sh, cfgs[0].batch_size, C, Ms, false, o)) || (rc = mlp_alloc(e, fresh, &block, Ms * k.stride)) ||
        (rc = mlp_alloc(e, fresh, &dmem, Ms)) || (rc = mlp_alloc(e, fresh, &smem, Ms)) || (rc = mlp_alloc(e, fresh, &cells, Ms * 4u)) ||
        (rc = mlp_alloc(e, fresh, &dsteps, Ms * 3u * (size_t)kTd3PopBlock))) {
        mlp_free(e, fresh);
        return rc;
    }
    td3_drop(e);
    e->td3_allocs.swap(fresh);
    off_install(e, o, sh);
    e->td3_cfg = sac_as_td3(cfgs[0]);
    e->sp_cfg.assign(Ms, cfgs[0]);
    if (count > 1) e->sp_cfg.assign(cfgs, cfgs + M);
    e->tp_cfg.resize(Ms);
    e->tp_mem.assign(Ms, Td3Member{});
    e->sp_mem.assign(Ms, SacMember{});
    e->tp_dmem = dmem; e->sp_dmem = smem; e->sp_cells = cells; e->tp_dsteps = dsteps; e->tp_part_stride = o.part_stride;
    std::vector<float> cell0(Ms * 4u, 0.0f);
    for (size_t m = 0; m < Ms; ++m) {
        e->tp_cfg[m] = sac_as_td3(e->sp_cfg[m]);
        sp_member_fill(e, m, e->sp_cfg[m]);
        e->sp_mem[m].cell = cells + m * 4u;
        off_member_place(e->tp_mem[m], m, k, 4, block, o, sh, C);
        const float la = adc::sac_log_alpha_init(e->sp_cfg[m].init_alpha);
        cell0[m * 4u + kSacCellLogAlpha] = la; cell0[m * 4u + kSacCellAlpha] = adc::mlp_exp(la);
    }
    // member 0's stores against the flat orders; theta's are the learners' policy layers
    tp_theta_layout(e, k.stride);
    off_layouts(e, e->tp_mem[0].q, e->tp_mem[0].q_t, e->tp_mem[0].pol_t);
    e->td3_a_shift = e->td3_a_scale = nullptr; e->td3_ring = Td3Ring{};
    e->tp_steps.assign(Ms * 3u * (size_t)kTd3PopBlock, Td3PopStep{});
    e->tp_host_sums.assign(Ms * 16u, 0.0);
    e->tp_critic_set.assign(Ms * kOffCriticFlags, 0);
    if ((rc = sp_members_upload(e))) return rc;
    HIP_TRY(hipMemcpyAsync(cells, cell0.data(), cell0.size() * 4, hipMemcpyHostToDevice, e->stream));
    // every member's theta starts as its device policy; the target critics as copies (zeros until the critics are uploaded and synchronised)
    tp_params_copy(e, kTd3Theta, 0, M, 1);
    if ((rc = off_sync_run(e, 0, M, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));       // (cell0 is the host's until here)
    e->have_sac_pop = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_set_critic_layer(adc_engine *e, int32_t member, int32_t critic, int32_t layer, const float *weights_in_out,
                                                   const float *bias_out)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_set_critic_layer(e, member, critic, layer, weights_in_out, bias_out);
}

ADC_EXPORT int adc_engine_sac_pop_sync_targets(adc_engine *e, int32_t member)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (member != -1 && (rc = tp_member_check(e, member)))) return rc;
    ENGINE_GUARD(e);
    if ((rc = member == -1 ? off_sync_run(e, 0, e->lrn_M, 1) : off_sync_run(e, member, 1, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_store(adc_engine *e, int64_t *stored_per_member)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = sp_state_check(e)) || (rc = off_store_check(e))) return rc;
    if (e->ro_teacher > 0) return fail(ADC_ESTATE, "the record holds teacher days: a soft actor-critic ring would need the pre-squash action of the teacher");
    ENGINE_GUARD(e);
    const long long count = (long long)(e->ro_t - e->td3_stored_t) * e->lrn_n;      // (a member's envs, not the engine's)
    // (raw rows under a running observation normaliser - SAC's set, e->sn: the last day's x' is the raw row an act would read now)
    // (with an observation history the last day's x' is the stacked row, peeked)
    if (e->nstep_n) off_store_nstep_launch(e, true, e->sn.obs.count != 0, count);       // (n-step returns: the window's R, done and gn)
    else if (e->mp.frames > 1)
        hipLaunchKernelGGL(k_td3_pop_store_hist, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, e->sn.obs.count ? nullptr : e->mp.shift,
                           e->sn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A,
                           e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem,
                           (unsigned long long)e->td3_written, (unsigned long long)e->td3_cfg.capacity,
                           e->mp.hist, e->mp.last, e->mp.from, e->mp.frames);
    else
        hipLaunchKernelGGL(k_td3_pop_store, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, e->sn.obs.count ? nullptr : e->mp.shift,
                           e->sn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A,
                           e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem,
                           (unsigned long long)e->td3_written, (unsigned long long)e->td3_cfg.capacity);
    return off_store_done(e, count, stored_per_member);
}

ADC_EXPORT int adc_engine_sac_pop_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity, int32_t *batch_size)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sp_ready(e)) return rc;
    return off_buffer_info(e, size, written, capacity, batch_size);
}

ADC_EXPORT int adc_engine_sac_pop_buffer_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done,
                                               float *x2)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_ring_fetch(e, member, slot, count, x, a, r, done, x2);
}

ADC_EXPORT int adc_engine_sac_pop_buffer_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *x, const float *a, const float *r,
                                              const uint8_t *done, const float *x2, int64_t written)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_ring_load(e, member, slot, count, x, a, r, done, x2, written);
}

ADC_EXPORT int adc_engine_sac_pop_batch_indices(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_batch_indices(e, e->tp_mem[(size_t)member].key, update, idx_b, "the replay buffer is empty (adc_engine_sac_pop_store)");
}

ADC_EXPORT int adc_engine_sac_pop_update(adc_engine *e, int32_t updates, adc_sac_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = sp_state_check(e)) ||
        (rc = off_update_check(e, updates, true, "a critic layer of a member has not been uploaded (adc_engine_sac_pop_set_critic_layer)",
                               "the replay buffer is empty (adc_engine_sac_pop_store)", 0x7FFFFFFFll)))
        return rc;
    ENGINE_GUARD(e);
    const int M = e->lrn_M;
    bool any_clip = false, any_alpha = false;
    for (const adc_sac_config &c : e->sp_cfg) { any_clip = any_clip || c.max_grad_norm > 0.0f; any_alpha = any_alpha || c.alpha_lr > 0.0f; }
    rc = off_pop_updates(
        e, updates, 3,
        [&](int nb) {
            for (int i = 0; i < nb; ++i) sp_steps_fill(e, i, e->td3_updates + i);
        },
        [&](int u, int i) { return sp_one_update(e, i, stats_m != nullptr, u + 1 == updates, any_clip, any_alpha); });
    if (rc) return rc;
    std::vector<float> cells;
    if (stats_m) {
        cells.resize((size_t)M * 4u);
        HIP_TRY(hipMemcpyAsync(e->tp_host_sums.data(), e->td3_sums, (size_t)M * 16 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(cells.data(), e->sp_cells, cells.size() * 4, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats_m)
        for (int m = 0; m < M; ++m) sac_stats_fill(e, e->tp_host_sums.data() + (size_t)m * 16, cells.data() + (size_t)m * 4u, stats_m + m);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sp_ready(e)) return rc;
    return off_param_counts(e, actor_p, critics_2qc);
}

ADC_EXPORT int adc_engine_sac_pop_state_get(adc_engine *e, int32_t member, float *theta_p, float *psi_q, float *psi_target_q, float *m_theta_p,
                                            float *v_theta_p, float *m_psi_q, float *v_psi_q, float *log_alpha3, int64_t *updates)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    float *flat[4] = {theta_p, psi_q, nullptr, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    if ((rc = off_state_get(e, member, flat, mom))) return rc;
    if (log_alpha3) HIP_TRY(hipMemcpyAsync(log_alpha3, e->sp_cells + (size_t)member * 4u, 3 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (updates) *updates = e->td3_updates;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_state_set(adc_engine *e, int32_t member, const float *theta_p, const float *psi_q, const float *psi_target_q,
                                            const float *m_theta_p, const float *v_theta_p, const float *m_psi_q, const float *v_psi_q,
                                            const float *log_alpha3, int64_t updates)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const float *flat[4] = {theta_p, psi_q, nullptr, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member)) || (rc = sac_state_set_check(flat, mom, log_alpha3, updates))) return rc;
    ENGINE_GUARD(e);
    float cell[4];
    if ((rc = sac_cell_upload(e, e->sp_cells + (size_t)member * 4u, log_alpha3, cell))) return rc;
    return off_state_set(e, member, flat, mom, updates);       // (waits: `cell` is the host's until then)
}

ADC_EXPORT int adc_engine_sac_pop_set_config(adc_engine *e, int32_t member, const adc_sac_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    const char *why = nullptr;
    if (adc_sac_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    const adc_sac_config shared[2] = {e->sp_cfg[0], *cfg};
    if (adc_sac_pop_config_check(shared, 2, 2, 2, &why) != ADC_OK)
        return fail(ADC_EINVAL, "batch_size, capacity, the critics' shape and target_update_interval may not change: the members' updates run in the same launches");
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));       // (an upload of the host's tables may still be in flight)
    // (init_alpha is not read again: the temperature cell is state)
    e->sp_cfg[(size_t)member] = *cfg;
    e->tp_cfg[(size_t)member] = sac_as_td3(*cfg);
    sp_member_fill(e, (size_t)member, *cfg);
    if ((rc = sp_members_upload(e))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_copy(adc_engine *e, int32_t src, int32_t dst, int32_t with_ring)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, src)) || (rc = tp_member_check(e, dst))) return rc;
    if (src == dst) return ADC_OK;
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->sp_cells + (size_t)dst * 4u, e->sp_cells + (size_t)src * 4u, 4 * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return off_pop_copy(e, src, dst, with_ring);
}
