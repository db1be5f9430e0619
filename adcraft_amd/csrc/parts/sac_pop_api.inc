// sac_pop_api.inc - the extern "C" entry points of SAC learner populations: M soft actor-critic learners in lock-step on one engine,
// every launch over all members (include/adcraft_engine.h; the kernels are parts/kernel_sac_pop.inc, the k_td3_pop_* of
// parts/kernel_td3_pop.inc and the k_pg_pop_* of parts/kernel_pg.inc; the law is csrc/adc_sac.h).  The population lives in the TD3
// population's engine fields and uses td3_pop_api.inc's helpers as they are (tp_params_copy, tp_csum_launch, tp_wgrad_launch,
// tp_step_run): td3_flat / td3_mom are [M][P] and [M][2 Qc] (no target actor), the scratch [M][B][...], td3_sums [M][16], tp_cfg
// what those helpers read of a member's configuration (sac_as_td3), the step table three rows per update (critic, actor,
// temperature).  What TD3 lacks - the law's SAC constants, the target entropy, the temperature cell - is in SacMember[M].
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
// the target critics of members member0 .. member0 + count - 1 become copies of their critics
int sp_sync_run(adc_engine *e, int member0, int count)
{
    const size_t Q2 = 2 * (size_t)e->td3_Qc, at = (size_t)member0 * Q2;
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3PsiT] + at, e->td3_flat[kTd3Psi] + at, (size_t)count * Q2 * 4, hipMemcpyDeviceToDevice, e->stream));
    tp_params_copy(e, kTd3PsiT, member0, count, 0);
    HIP_TRY(hipGetLastError());
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
    const adc::Td3Shape sh = adc::sac_shape_of(e->mlp_cfg, e->v.K, cfgs[0]);
    if (sac_lds_floats(sh) * sizeof(float) > 64u * 1024u) return fail(ADC_EINVAL, "num_keywords too large for soft actor-critic training (LDS)");
    ENGINE_GUARD(e);
    const int A = sh.A, D = sh.D, B = cfgs[0].batch_size;
    const size_t Ms = (size_t)M, C = (size_t)cfgs[0].capacity, P = (size_t)adc::td3_params(sh.pol), Qc = (size_t)adc::td3_params(sh.q), Q2 = 2 * Qc,
                 Qmax = std::max(P, Q2);
    const size_t na = (size_t)std::max(std::max(2 * adc::td3_hidden(sh.q), adc::td3_hidden(sh.pol)), 1);
    const size_t nd = (size_t)std::max(2 * adc::td3_outs(sh.q), adc::td3_outs(sh.pol));
    const size_t part_stride = (size_t)pg_chunks((long long)std::max((size_t)B, Qmax)) * 8u + 8u;
    // a member's block of stores: critic 1, critic 2, target critic 1, target critic 2, every piece on a 16-byte boundary
    size_t offW[4][adc::kMlpMaxLayers] = {}, offb[4][adc::kMlpMaxLayers] = {}, stride = 0;
    for (int n = 0; n < 4; ++n)
        for (int l = 0; l < sh.q.layers; ++l) {
            offW[n][l] = stride; stride += adc::mlp_weight_count(adc::td3_n_in(sh.q, l), sh.q.n_out[l]);
            offb[n][l] = stride; stride += ((size_t)sh.q.n_out[l] + 3u) & ~(size_t)3u;
        }
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    int rc = ADC_OK;
    float *block = nullptr, *flat[4] = {}, *mom[4] = {}, *grad = nullptr, *ybuf = nullptr, *xin = nullptr, *acts = nullptr, *deltas = nullptr, *pieces = nullptr,
          *rx = nullptr, *ra = nullptr, *rr = nullptr, *rx2 = nullptr, *cells = nullptr;
    uint8_t *rdone = nullptr;
    int32_t *idx = nullptr;
    double *part = nullptr, *sums = nullptr, *gpart = nullptr;
    Td3Member *dmem = nullptr;
    SacMember *smem = nullptr;
    Td3PopStep *dsteps = nullptr;
    for (int w = 0; w < 4 && !rc; ++w) {
        if (w != kTd3ThetaT) rc = mlp_alloc(e, fresh, &flat[w], Ms * ((w & 1) ? Q2 : P));
        if (!rc) rc = mlp_alloc(e, fresh, &mom[w], Ms * (w < 2 ? P : Q2));
    }
    if (rc || (rc = mlp_alloc(e, fresh, &block, Ms * stride)) || (rc = mlp_alloc(e, fresh, &grad, Ms * Qmax)) || (rc = mlp_alloc(e, fresh, &ybuf, Ms * (size_t)B)) ||
        (rc = mlp_alloc(e, fresh, &xin, Ms * (size_t)B * (size_t)(D + A))) || (rc = mlp_alloc(e, fresh, &acts, Ms * (size_t)B * na)) ||
        (rc = mlp_alloc(e, fresh, &deltas, Ms * (size_t)B * nd)) || (rc = mlp_alloc(e, fresh, &pieces, Ms * (size_t)B * (size_t)adc::kTd3Pieces)) ||
        (rc = mlp_alloc(e, fresh, &idx, (size_t)B)) || (rc = mlp_alloc(e, fresh, &part, Ms * part_stride)) || (rc = mlp_alloc(e, fresh, &sums, Ms * 16u)) ||
        (rc = mlp_alloc(e, fresh, &gpart, Ms * (size_t)pg_chunks(B) * Qmax)) || (rc = mlp_alloc(e, fresh, &rx, Ms * C * (size_t)D)) ||
        (rc = mlp_alloc(e, fresh, &ra, Ms * C * (size_t)A)) || (rc = mlp_alloc(e, fresh, &rr, Ms * C)) || (rc = mlp_alloc(e, fresh, &rdone, Ms * C)) ||
        (rc = mlp_alloc(e, fresh, &rx2, Ms * C * (size_t)D)) || (rc = mlp_alloc(e, fresh, &dmem, Ms)) || (rc = mlp_alloc(e, fresh, &smem, Ms)) ||
        (rc = mlp_alloc(e, fresh, &cells, Ms * 4u)) || (rc = mlp_alloc(e, fresh, &dsteps, Ms * 3u * (size_t)kTd3PopBlock))) {
        mlp_free(e, fresh);
        return rc;
    }
    td3_drop(e);
    e->td3_allocs.swap(fresh);
    e->td3_cfg = sac_as_td3(cfgs[0]); e->td3_shape = sh;
    e->td3_P = (int)P; e->td3_Qc = (int)Qc;
    e->sp_cfg.assign(Ms, cfgs[0]);
    if (count > 1) e->sp_cfg.assign(cfgs, cfgs + M);
    e->tp_cfg.resize(Ms);
    e->tp_mem.assign(Ms, Td3Member{});
    e->sp_mem.assign(Ms, SacMember{});
    e->tp_dmem = dmem; e->sp_dmem = smem; e->sp_cells = cells; e->tp_dsteps = dsteps; e->tp_part_stride = part_stride;
    std::vector<float> cell0(Ms * 4u, 0.0f);
    for (size_t m = 0; m < Ms; ++m) {
        Td3Member &me = e->tp_mem[m];
        e->tp_cfg[m] = sac_as_td3(e->sp_cfg[m]);
        sp_member_fill(e, m, e->sp_cfg[m]);
        e->sp_mem[m].cell = cells + m * 4u;
        float *base = block + m * stride;
        MlpNet *nets[4] = {&me.q[0], &me.q[1], &me.q_t[0], &me.q_t[1]};
        for (int n = 0; n < 4; ++n) {
            nets[n]->layers = sh.q.layers;
            for (int l = 0; l < sh.q.layers; ++l) {
                nets[n]->W[l] = base + offW[n][l]; nets[n]->b[l] = base + offb[n][l];
                nets[n]->n_in[l] = adc::td3_n_in(sh.q, l); nets[n]->n_out[l] = sh.q.n_out[l];
            }
        }
        me.ring = Td3Ring{rx + m * C * (size_t)D, ra + m * C * (size_t)A, rr + m * C, rx2 + m * C * (size_t)D, rdone + m * C};
        const float la = adc::sac_log_alpha_init(e->sp_cfg[m].init_alpha);
        cell0[m * 4u + kSacCellLogAlpha] = la; cell0[m * 4u + kSacCellAlpha] = adc::mlp_exp(la);
    }
    // member 0's stores against the flat orders; theta's are the learners' policy layers
    e->td3_lay[kTd3Theta] = e->lrn_lay;
    e->td3_lay[kTd3Theta].nterms = sh.pol.layers; e->td3_lay[kTd3Theta].Q = (int)P;
    e->td3_lay[kTd3Psi] = td3_layout(e->tp_mem[0].q, 2);
    e->td3_lay[kTd3ThetaT] = PgLayout{};
    e->td3_lay[kTd3PsiT] = td3_layout(e->tp_mem[0].q_t, 2);
    e->tp_stride[kTd3Theta] = e->lrn_stride;
    e->tp_stride[kTd3Psi] = e->tp_stride[kTd3ThetaT] = e->tp_stride[kTd3PsiT] = stride;
    for (int w = 0; w < 4; ++w) { e->td3_flat[w] = flat[w]; e->td3_mom[w] = mom[w]; }
    e->td3_a_shift = e->td3_a_scale = nullptr; e->td3_ring = Td3Ring{};
    e->td3_grad = grad; e->td3_ybuf = ybuf; e->td3_xin = xin; e->td3_acts = acts; e->td3_deltas = deltas; e->td3_pieces = pieces; e->td3_idx = idx;
    e->td3_part = part; e->td3_sums = sums; e->td3_gpart = gpart;
    e->tp_steps.assign(Ms * 3u * (size_t)kTd3PopBlock, Td3PopStep{});
    e->tp_host_sums.assign(Ms * 16u, 0.0);
    e->tp_critic_set.assign(Ms * 2u * adc::kMlpMaxLayers, 0);
    e->td3_stored_t = e->ro_t;              // (days recorded before this call are not the trainer's)
    if ((rc = sp_members_upload(e))) return rc;
    HIP_TRY(hipMemcpyAsync(cells, cell0.data(), cell0.size() * 4, hipMemcpyHostToDevice, e->stream));
    // every member's theta starts as its device policy; the target critics as copies (zeros until the critics are uploaded and synchronised)
    tp_params_copy(e, kTd3Theta, 0, M, 1);
    if ((rc = sp_sync_run(e, 0, M))) return rc;
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
    if (critic != 0 && critic != 1) return fail(ADC_EINVAL, "critic: 0 or 1");
    const adc::Td3Net &q = e->td3_shape.q;
    if (layer < 0 || layer >= q.layers) return fail(ADC_EINVAL, "no such critic layer");
    if (!weights_in_out || !bias_out) return fail(ADC_EINVAL, "weights or bias is NULL");
    ENGINE_GUARD(e);
    size_t off = (size_t)member * 2u * (size_t)e->td3_Qc + (size_t)critic * (size_t)e->td3_Qc;
    for (int l = 0; l < layer; ++l) off += (size_t)(adc::td3_n_in(q, l) + 1) * (size_t)q.n_out[l];
    const size_t nw = (size_t)adc::td3_n_in(q, layer) * (size_t)q.n_out[layer];
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3Psi] + off, weights_in_out, nw * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3Psi] + off + nw, bias_out, (size_t)q.n_out[layer] * 4, hipMemcpyHostToDevice, e->stream));
    tp_params_copy(e, kTd3Psi, member, 1, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->tp_critic_set[((size_t)member * 2u + (size_t)critic) * adc::kMlpMaxLayers + (size_t)layer] = 1;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_sync_targets(adc_engine *e, int32_t member)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (member != -1 && (rc = tp_member_check(e, member)))) return rc;
    ENGINE_GUARD(e);
    if ((rc = member == -1 ? sp_sync_run(e, 0, e->lrn_M) : sp_sync_run(e, member, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_store(adc_engine *e, int64_t *stored_per_member)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = sp_state_check(e))) return rc;
    if (e->ro_t <= e->td3_stored_t) return fail(ADC_ESTATE, "no unstored day in the record (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    if (e->td3_gap || e->env_moves != e->ro_moves)
        return fail(ADC_ESTATE, "the envs were stepped or reset outside the record since an unstored recorded day: its next observation is not the "
                                "one the envs hold (adc_engine_rollout_reset, collect again)");
    ENGINE_GUARD(e);
    const long long count = (long long)(e->ro_t - e->td3_stored_t) * e->lrn_n;
    // (raw rows under a running observation normaliser: the last day's x' is the raw row an act would read now)
    hipLaunchKernelGGL(k_td3_pop_store, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, e->sn.obs.count ? nullptr : e->mp.shift,
                       e->sn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A,
                       e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem,
                       (unsigned long long)e->td3_written, (unsigned long long)e->td3_cfg.capacity);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_store_run(e, e->td3_written, count))) return rc;
    e->td3_written += count;
    e->td3_stored_t = e->ro_t;
    if (stored_per_member) *stored_per_member = count;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity, int32_t *batch_size)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sp_ready(e)) return rc;
    if (size) *size = td3_size(e);
    if (written) *written = e->td3_written;
    if (capacity) *capacity = e->td3_cfg.capacity;
    if (batch_size) *batch_size = e->td3_cfg.batch_size;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_buffer_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done,
                                               float *x2)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    if (slot < 0 || count < 1 || slot > td3_size(e) - count) return fail(ADC_EINVAL, "the slot range is not inside [0, size)");
    ENGINE_GUARD(e);
    const size_t s = (size_t)slot, n = (size_t)count, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
    const Td3Ring &g = e->tp_mem[(size_t)member].ring;
    if (x) HIP_TRY(hipMemcpyAsync(x, g.x + s * D, n * D * 4, hipMemcpyDeviceToHost, e->stream));
    if (a) HIP_TRY(hipMemcpyAsync(a, g.a + s * A, n * A * 4, hipMemcpyDeviceToHost, e->stream));
    if (r) HIP_TRY(hipMemcpyAsync(r, g.r + s, n * 4, hipMemcpyDeviceToHost, e->stream));
    if (done) HIP_TRY(hipMemcpyAsync(done, g.done + s, n, hipMemcpyDeviceToHost, e->stream));
    if (x2) HIP_TRY(hipMemcpyAsync(x2, g.x2 + s * D, n * D * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_buffer_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *x, const float *a, const float *r,
                                              const uint8_t *done, const float *x2, int64_t written)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    if (!x || !a || !r || !done || !x2) return fail(ADC_EINVAL, "x, a, r, done or x2 is NULL");
    if (slot < 0 || count < 1 || slot > (int64_t)e->td3_cfg.capacity - count) return fail(ADC_EINVAL, "the slot range is not inside [0, capacity)");
    if (written < slot + count) return fail(ADC_EINVAL, "written: at least slot + count");
    ENGINE_GUARD(e);
    const size_t s = (size_t)slot, n = (size_t)count, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
    const Td3Ring &g = e->tp_mem[(size_t)member].ring;
    HIP_TRY(hipMemcpyAsync(g.x + s * D, x, n * D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.a + s * A, a, n * A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.r + s, r, n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.done + s, done, n, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.x2 + s * D, x2, n * D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_written = written;               // (the members' rings move together: one count for all)
    if (e->per_live) {
        if ((rc = per_loaded_run(e, member, slot, count))) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_batch_indices(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    if (!idx_b) return fail(ADC_EINVAL, "idx_b is NULL");
    if (update < 0 || update >= 0xFFFFFFFFll) return fail(ADC_EINVAL, "update: 0 to 2^32 - 2");
    if (td3_size(e) == 0) return fail(ADC_ESTATE, "the replay buffer is empty (adc_engine_sac_pop_store)");
    if (e->per_live) return fail(ADC_ESTATE, "prioritised replay is alive on this engine: the batch is adc_engine_replay_prio_batch's, not the uniform law's");
    ENGINE_GUARD(e);
    const int B = e->td3_cfg.batch_size;
    hipLaunchKernelGGL(k_td3_indices, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, e->stream, e->tp_mem[(size_t)member].key, (uint32_t)update,
                       (uint32_t)td3_size(e), B, e->td3_idx);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx_b, e->td3_idx, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_update(adc_engine *e, int32_t updates, adc_sac_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = sp_state_check(e))) return rc;
    if (updates < 1 || updates > 65536) return fail(ADC_EINVAL, "updates: 1 to 65536");
    if (!tp_critics_set(e)) return fail(ADC_ESTATE, "a critic layer of a member has not been uploaded (adc_engine_sac_pop_set_critic_layer)");
    if (td3_size(e) == 0) return fail(ADC_ESTATE, "the replay buffer is empty (adc_engine_sac_pop_store)");
    if (e->td3_updates + updates >= 0x7FFFFFFFll) return fail(ADC_ESTATE, "the update counter is exhausted");
    ENGINE_GUARD(e);
    const int M = e->lrn_M;
    bool any_clip = false, any_alpha = false;
    for (const adc_sac_config &c : e->sp_cfg) { any_clip = any_clip || c.max_grad_norm > 0.0f; any_alpha = any_alpha || c.alpha_lr > 0.0f; }
    HIP_TRY(hipMemsetAsync(e->td3_sums, 0, (size_t)M * 16 * sizeof(double), e->stream));
    for (int u0 = 0; u0 < updates; u0 += kTd3PopBlock) {
        const int nb = std::min(kTd3PopBlock, updates - u0);
        // the block's step constants (the Adam bias corrections of every step to come) in one copy; the host's table is free to
        // write: the call before this one, and the block before this one, ended with a wait
        if (u0 > 0) HIP_TRY(hipStreamSynchronize(e->stream));
        for (int i = 0; i < nb; ++i) sp_steps_fill(e, i, e->td3_updates + i);
        HIP_TRY(hipMemcpyAsync(e->tp_dsteps, e->tp_steps.data(), (size_t)nb * 3u * (size_t)M * sizeof(Td3PopStep), hipMemcpyHostToDevice, e->stream));
        for (int i = 0; i < nb; ++i)
            if ((rc = sp_one_update(e, i, stats_m != nullptr, u0 + i + 1 == updates, any_clip, any_alpha))) return rc;
    }
    std::vector<float> cells;
    if (stats_m) {
        cells.resize((size_t)M * 4u);
        HIP_TRY(hipMemcpyAsync(e->tp_host_sums.data(), e->td3_sums, (size_t)M * 16 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(cells.data(), e->sp_cells, cells.size() * 4, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats_m) {
        const double n = (double)e->td3_cfg.batch_size;
        for (int m = 0; m < M; ++m) {
            const double *sums = e->tp_host_sums.data() + (size_t)m * 16;
            const float *cell = cells.data() + (size_t)m * 4u;
            adc_sac_stats *stats = stats_m + m;
            const double l1 = sums[adc::kTd3Loss1] / n, l2 = sums[adc::kTd3Loss2] / n;
            stats->updates = e->td3_updates; stats->buffer_size = td3_size(e); stats->samples = e->td3_cfg.batch_size;
            stats->critic_loss = l1 + l2;
            stats->q1_mean = sums[adc::kTd3Q1] / n; stats->q2_mean = sums[adc::kTd3Q2] / n; stats->y_mean = sums[adc::kTd3Y] / n;
            stats->actor_loss = sums[adc::kSacPiLoss] / n;
            stats->logp_mean = sums[adc::kSacLp] / n;
            stats->alpha = cell[kSacCellAlpha]; stats->log_alpha = cell[kSacCellLogAlpha];
            stats->critic_grad_norm = std::sqrt(sums[8]);
            stats->actor_grad_norm = std::sqrt(sums[9]);
        }
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sp_ready(e)) return rc;
    if (actor_p) *actor_p = e->td3_P;
    if (critics_2qc) *critics_2qc = 2 * (int64_t)e->td3_Qc;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_state_get(adc_engine *e, int32_t member, float *theta_p, float *psi_q, float *psi_target_q, float *m_theta_p,
                                            float *v_theta_p, float *m_psi_q, float *v_psi_q, float *log_alpha3, int64_t *updates)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    const size_t P = (size_t)e->td3_P, Q2 = 2 * (size_t)e->td3_Qc, mi = (size_t)member;
    float *flat[4] = {theta_p, psi_q, nullptr, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    for (int w = 0; w < 4; ++w) {
        const size_t fq = (w & 1) ? Q2 : P, mq = w < 2 ? P : Q2;
        if (flat[w]) HIP_TRY(hipMemcpyAsync(flat[w], e->td3_flat[w] + mi * fq, fq * 4, hipMemcpyDeviceToHost, e->stream));
        if (mom[w]) HIP_TRY(hipMemcpyAsync(mom[w], e->td3_mom[w] + mi * mq, mq * 4, hipMemcpyDeviceToHost, e->stream));
    }
    if (log_alpha3) HIP_TRY(hipMemcpyAsync(log_alpha3, e->sp_cells + mi * 4u, 3 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (updates) *updates = e->td3_updates;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_pop_state_set(adc_engine *e, int32_t member, const float *theta_p, const float *psi_q, const float *psi_target_q,
                                            const float *m_theta_p, const float *v_theta_p, const float *m_psi_q, const float *v_psi_q,
                                            const float *log_alpha3, int64_t updates)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    if (!theta_p || !psi_q || !psi_target_q || !m_theta_p || !v_theta_p || !m_psi_q || !v_psi_q || !log_alpha3) return fail(ADC_EINVAL, "a state vector is NULL");
    if (updates < 0 || updates >= 0x7FFFFFFFll) return fail(ADC_EINVAL, "updates: 0 to 2^31 - 2");
    if (!std::isfinite(log_alpha3[0])) return fail(ADC_EINVAL, "log_alpha must be finite");
    ENGINE_GUARD(e);
    const size_t P = (size_t)e->td3_P, Q2 = 2 * (size_t)e->td3_Qc, mi = (size_t)member;
    const float *flat[4] = {theta_p, psi_q, nullptr, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    for (int w = 0; w < 4; ++w) {
        const size_t fq = (w & 1) ? Q2 : P, mq = w < 2 ? P : Q2;
        HIP_TRY(hipMemcpyAsync(e->td3_mom[w] + mi * mq, mom[w], mq * 4, hipMemcpyHostToDevice, e->stream));
        if (!flat[w]) continue;
        HIP_TRY(hipMemcpyAsync(e->td3_flat[w] + mi * fq, flat[w], fq * 4, hipMemcpyHostToDevice, e->stream));
        tp_params_copy(e, w, member, 1, 0);         // (the member's policy layers, critics and target critics follow its flat vectors)
    }
    const float cell[4] = {log_alpha3[0], log_alpha3[1], log_alpha3[2], adc::mlp_exp(log_alpha3[0])};
    HIP_TRY(hipMemcpyAsync(e->sp_cells + mi * 4u, cell, sizeof(cell), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_updates = updates;                       // (the members move together: one counter for all)
    for (size_t i = 0; i < 2u * adc::kMlpMaxLayers; ++i) e->tp_critic_set[mi * 2u * adc::kMlpMaxLayers + i] = 1;
    return ADC_OK;
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
    const size_t P = (size_t)e->td3_P, Q2 = 2 * (size_t)e->td3_Qc, from = (size_t)src, to = (size_t)dst;
    for (int w = 0; w < 4; ++w) {
        const size_t fq = (w & 1) ? Q2 : P, mq = w < 2 ? P : Q2;
        HIP_TRY(hipMemcpyAsync(e->td3_mom[w] + to * mq, e->td3_mom[w] + from * mq, mq * 4, hipMemcpyDeviceToDevice, e->stream));
        if (w == kTd3ThetaT) continue;
        HIP_TRY(hipMemcpyAsync(e->td3_flat[w] + to * fq, e->td3_flat[w] + from * fq, fq * 4, hipMemcpyDeviceToDevice, e->stream));
        tp_params_copy(e, w, dst, 1, 0);
    }
    HIP_TRY(hipMemcpyAsync(e->sp_cells + to * 4u, e->sp_cells + from * 4u, 4 * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipGetLastError());
    if (with_ring) {
        const size_t C = (size_t)e->td3_cfg.capacity, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
        const Td3Ring &s = e->tp_mem[from].ring, &d = e->tp_mem[to].ring;
        HIP_TRY(hipMemcpyAsync(d.x, s.x, C * D * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.a, s.a, C * A * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.r, s.r, C * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.done, s.done, C, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.x2, s.x2, C * D * 4, hipMemcpyDeviceToDevice, e->stream));
        if (e->per_live && (rc = per_copy_run(e, src, dst))) return rc;     // (the leaves, nodes and top travel with the ring)
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t per = 2u * adc::kMlpMaxLayers;
    for (size_t i = 0; i < per; ++i) e->tp_critic_set[to * per + i] = e->tp_critic_set[from * per + i];
    return ADC_OK;
}
