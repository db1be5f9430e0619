// td3_api.inc - the extern "C" entry points of off-policy (TD3) training (include/adcraft_engine.h; the kernels are
// parts/kernel_td3.inc, the law csrc/adc_td3.h).  Everything here runs on the engine's own stream behind ENGINE_GUARD, that is
// after the env groups have joined: results do not depend on how the days were grouped.
// (part of the single translation unit adc_engine.hip)
namespace {
// prioritised replay's side of an update, a store, a buffer load and a member copy (parts/per_api.inc; called only while e->per_live)
int per_sample_run(adc_engine *e, uint32_t update);
int per_leaves_run(adc_engine *e);
int per_store_run(adc_engine *e, int64_t written_before, int64_t count);
int per_loaded_run(adc_engine *e, int member, int64_t slot, int64_t count);
int per_copy_run(adc_engine *e, int src, int dst);
void per_pairs_launch(adc_engine *e, int npairs);
enum { kTd3Theta = 0, kTd3Psi = 1, kTd3ThetaT = 2, kTd3PsiT = 3 };

int td3_ready(const adc_engine *e)
{
    if (!e->have_td3) return fail(ADC_ESTATE, "adc_engine_td3_init has not been called (or the policy / the record was re-initialised since)");
    return ADC_OK;
}
// what an off-policy call needs of the engine's state, checked at init and again at every call
int td3_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (e->mp.two_heads) return fail(ADC_ESTATE, "TD3 needs the policy with the free log_std head: a two-headed policy (2A outputs) is not supported");
    if (e->pop_M != 0) return fail(ADC_ESTATE, "off-policy training with a population active is not supported (adc_engine_mlp_population(0) first)");
    if (e->lrn_M != 0) return fail(ADC_ESTATE, "off-policy training with learners active is not supported (adc_engine_mlp_learners(0) first)");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "off-policy training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "off-policy training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
inline int64_t td3_size(const adc_engine *e) { return std::min<int64_t>(e->td3_written, (int64_t)e->td3_cfg.capacity); }

// the flat order of `count` networks' layers against their chain-major stores
PgLayout td3_layout(const MlpNet *nets, int count)
{
    PgLayout lay{};
    int flat = 0, i = 0;
    for (int n = 0; n < count; ++n)
        for (int l = 0; l < nets[n].layers; ++l, ++i) {
            lay.flat0[i] = flat; lay.n_in[i] = nets[n].n_in[l]; lay.n_out[i] = nets[n].n_out[l];
            lay.W[i] = const_cast<float *>(nets[n].W[l]); lay.b[i] = const_cast<float *>(nets[n].b[l]);
            flat += (nets[n].n_in[l] + 1) * nets[n].n_out[l];
        }
    lay.nterms = i; lay.Q = flat;
    return lay;
}
// which = 1: flat <- stores; 0: stores <- flat
void td3_params_copy(adc_engine *e, int which, int to_flat)
{
    const PgLayout &lay = e->td3_lay[which];
    hipLaunchKernelGGL(k_pg_params_copy, dim3((unsigned)((lay.Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, lay, e->td3_flat[which], to_flat);
}
int td3_sync_run(adc_engine *e)
{
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3ThetaT], e->td3_flat[kTd3Theta], (size_t)e->td3_P * 4, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3PsiT], e->td3_flat[kTd3Psi], (size_t)e->td3_Qc * 8, hipMemcpyDeviceToDevice, e->stream));
    td3_params_copy(e, kTd3ThetaT, 0);
    td3_params_copy(e, kTd3PsiT, 0);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
int td3_csum_launch(adc_engine *e, const float *src, long long n, int stride, int cols, int mode, double *out)
{
    const long long chunks = pg_chunks(n), lanes = chunks * cols;
    hipLaunchKernelGGL(k_pg_chunk_sums, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream, src, n, stride, cols, mode, 0.0, e->td3_part);
    hipLaunchKernelGGL(k_pg_join, dim3(1), dim3(64), 0, e->stream, e->td3_part, chunks, cols, out);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
adc::EsStep td3_step_of(const adc_td3_config &c, float lr, int64_t steps_taken)
{
    adc::EsStep step{};
    step.optimiser = c.optimiser == ADC_TD3_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = lr; step.beta1 = c.beta1; step.beta2 = c.beta2; step.eps = c.eps; step.l2 = 0.0f;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(steps_taken + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(steps_taken + 1));
    return step;
}
// the running normalisers' side of a batch kernel's view (all null without adc_engine_td3_norm_init: the kernels are what they were)
void td3_norm_fill(const adc_engine *e, Td3View &p)
{
    if (!e->tn.live) return;
    if (e->tn.obs.count) { p.n_shift = e->mp.shift; p.n_scale = e->mp.scale; p.n_stride = e->mp.norm_stride; }
    if (e->tn.rew.count) { p.r_scale = e->tn.rew.scale; p.r_stride = e->tn_cfg.per_member ? 1 : 0; p.r_clip = e->tn_cfg.rew_clip; }
}
// prioritised replay's side of a batch kernel's view (all null without adc_engine_replay_prio_init: the kernels are what they were)
template <class BatchView>
void td3_per_fill(const adc_engine *e, BatchView &p)
{
    if (!e->per_live) return;
    p.p_slot = e->per.slot; p.p_w = e->per.w; p.p_absd = e->per.absd;
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
// the weight gradient's partials of one network over the batch: its first layer's X is the gathered rows
void td3_wgrad_launch(adc_engine *e, const adc::Td3Net &net, int ldx0, int na, int acts_off, int nd, int d_off, int flat0, int Q, int B)
{
    int flat = flat0, ao = acts_off, dof = d_off;
    for (int l = 0; l < net.layers; ++l) {
        const int n_in = adc::td3_n_in(net, l), n_out = net.n_out[l];
        PgTerm t{l == 0 ? e->td3_xin : e->td3_acts + ao, l == 0 ? (size_t)ldx0 : (size_t)na, n_in, n_out, dof, flat, 0};
        const unsigned tiles = (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile));
        hipLaunchKernelGGL(k_pg_wgrad, dim3(tiles, (unsigned)pg_chunks(B)), dim3(kPgBlock), 0, e->stream, t, (long long)B, 1, 1, 0, e->td3_deltas, nd,
                           e->td3_gpart, Q);
        flat += (n_in + 1) * n_out;
        dof += n_out;
        if (l > 0) ao += n_in;
    }
}
// the gradient in td3_grad from the partials, its squared norm into sums[slot] when asked for, the clip's scale, the step
int td3_step_run(adc_engine *e, int which, float **mom, int Q, int B, bool norm_wanted, int slot, float lr, int64_t steps_taken)
{
    hipLaunchKernelGGL(k_pg_grad_join, dim3((unsigned)((Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->td3_gpart, (int)pg_chunks(B), Q,
                       (long long)B, e->td3_grad);
    HIP_TRY(hipGetLastError());
    const bool clip = e->td3_cfg.max_grad_norm > 0.0f;
    float scale = 1.0f;
    if (clip || norm_wanted)
        if (int rc = td3_csum_launch(e, e->td3_grad, Q, 1, 1, 2, e->td3_sums + slot)) return rc;
    if (clip) {
        double sq = 0.0;
        HIP_TRY(hipMemcpyAsync(&sq, e->td3_sums + slot, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        scale = adc::pg_clip_scale(e->td3_cfg.max_grad_norm, std::sqrt(sq));
    }
    hipLaunchKernelGGL(k_pg_update, dim3((unsigned)((Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->td3_lay[which], e->td3_flat[which],
                       mom[0], mom[1], e->td3_grad, clip ? 1 : 0, scale, td3_step_of(e->td3_cfg, lr, steps_taken));
    HIP_TRY(hipGetLastError());
    return ADC_OK;
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
    hipLaunchKernelGGL(k_td3_target, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    hipLaunchKernelGGL(k_td3_critic_sample, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    for (int i = 0; i < 2; ++i) td3_wgrad_launch(e, sh.q, DA, p.na, i * nh, p.nd, i * no, i * e->td3_Qc, 2 * e->td3_Qc, B);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_leaves_run(e))) return rc;
    if (stats_wanted && last && (rc = td3_csum_launch(e, e->td3_pieces, B, adc::kTd3Pieces, 5, 0, e->td3_sums))) return rc;
    if ((rc = td3_step_run(e, kTd3Psi, e->td3_mom + 2, 2 * e->td3_Qc, B, stats_wanted && last, 5, c.critic_lr, e->td3_updates))) return rc;
    if ((e->td3_updates + 1) % c.policy_delay == 0) {
        p.na = ph; p.nd = po;
        hipLaunchKernelGGL(k_td3_actor_sample, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
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
    const adc::Td3Shape sh = adc::td3_shape_of(e->mlp_cfg, e->v.K, *cfg, 0);
    if (td3_lds_floats(sh) * sizeof(float) > 64u * 1024u) return fail(ADC_EINVAL, "num_keywords too large for off-policy training (LDS)");
    ENGINE_GUARD(e);
    const int A = sh.A, D = sh.D, B = cfg->batch_size;
    const size_t C = (size_t)cfg->capacity, P = (size_t)adc::td3_params(sh.pol), Qc = (size_t)adc::td3_params(sh.q), Q2 = 2 * Qc, Qmax = std::max(P, Q2);
    const size_t na = (size_t)std::max(std::max(2 * adc::td3_hidden(sh.q), adc::td3_hidden(sh.pol)), 1);
    const size_t nd = (size_t)std::max(2 * adc::td3_outs(sh.q), adc::td3_outs(sh.pol));
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    int rc = ADC_OK;
    MlpNet nets[5] = {};                    // critic 1, critic 2, target critic 1, target critic 2, target actor
    for (int n = 0; n < 5 && !rc; ++n) {
        const adc::Td3Net &shape = n < 4 ? sh.q : sh.pol;
        nets[n].layers = shape.layers;
        for (int l = 0; l < shape.layers && !rc; ++l) {
            float *w = nullptr, *b = nullptr;
            const int n_in = adc::td3_n_in(shape, l), n_out = shape.n_out[l];
            if ((rc = mlp_alloc(e, fresh, &w, adc::mlp_weight_count(n_in, n_out))) || (rc = mlp_alloc(e, fresh, &b, (size_t)n_out))) break;
            nets[n].W[l] = w; nets[n].b[l] = b; nets[n].n_in[l] = n_in; nets[n].n_out[l] = n_out;
        }
    }
    float *flat[4] = {}, *mom[4] = {}, *shift = nullptr, *scale = nullptr, *grad = nullptr, *ybuf = nullptr, *xin = nullptr, *acts = nullptr, *deltas = nullptr,
          *pieces = nullptr;
    Td3Ring ring{};
    int32_t *idx = nullptr;
    double *part = nullptr, *sums = nullptr, *gpart = nullptr;
    for (int w = 0; w < 4 && !rc; ++w)
        if (!(rc = mlp_alloc(e, fresh, &flat[w], (w & 1) ? Q2 : P))) rc = mlp_alloc(e, fresh, &mom[w], w < 2 ? P : Q2);
    if (rc || (rc = mlp_alloc(e, fresh, &shift, (size_t)A)) || (rc = mlp_alloc(e, fresh, &scale, (size_t)A)) || (rc = mlp_alloc(e, fresh, &grad, Qmax)) ||
        (rc = mlp_alloc(e, fresh, &ybuf, (size_t)B)) || (rc = mlp_alloc(e, fresh, &xin, (size_t)B * (size_t)(D + A))) ||
        (rc = mlp_alloc(e, fresh, &acts, (size_t)B * na)) || (rc = mlp_alloc(e, fresh, &deltas, (size_t)B * nd)) ||
        (rc = mlp_alloc(e, fresh, &pieces, (size_t)B * (size_t)adc::kTd3Pieces)) || (rc = mlp_alloc(e, fresh, &idx, (size_t)B)) ||
        (rc = mlp_alloc(e, fresh, &part, (size_t)pg_chunks((long long)std::max((size_t)B, Qmax)) * 8u + 8u)) || (rc = mlp_alloc(e, fresh, &sums, (size_t)16)) ||
        (rc = mlp_alloc(e, fresh, &gpart, (size_t)pg_chunks(B) * Qmax)) || (rc = mlp_alloc(e, fresh, &ring.x, C * (size_t)D)) ||
        (rc = mlp_alloc(e, fresh, &ring.a, C * (size_t)A)) || (rc = mlp_alloc(e, fresh, &ring.r, C)) || (rc = mlp_alloc(e, fresh, &ring.done, C)) ||
        (rc = mlp_alloc(e, fresh, &ring.x2, C * (size_t)D))) {
        mlp_free(e, fresh);
        return rc;
    }
    td3_drop(e);
    e->td3_allocs.swap(fresh);
    e->td3_cfg = *cfg; e->td3_shape = sh;
    e->td3_key = adc::td3_key(cfg->seed ? cfg->seed : e->cfg.seed);
    e->td3_P = (int)P; e->td3_Qc = (int)Qc;
    e->td3_q[0] = nets[0]; e->td3_q[1] = nets[1]; e->td3_q_t[0] = nets[2]; e->td3_q_t[1] = nets[3]; e->td3_pol_t = nets[4];
    e->td3_lay[kTd3Theta] = td3_layout(&e->mp.pol, 1);
    e->td3_lay[kTd3Psi] = td3_layout(e->td3_q, 2);
    e->td3_lay[kTd3ThetaT] = td3_layout(&e->td3_pol_t, 1);
    e->td3_lay[kTd3PsiT] = td3_layout(e->td3_q_t, 2);
    for (int w = 0; w < 4; ++w) { e->td3_flat[w] = flat[w]; e->td3_mom[w] = mom[w]; }
    e->td3_a_shift = shift; e->td3_a_scale = scale; e->td3_ring = ring;
    e->td3_grad = grad; e->td3_ybuf = ybuf; e->td3_xin = xin; e->td3_acts = acts; e->td3_deltas = deltas; e->td3_pieces = pieces; e->td3_idx = idx;
    e->td3_part = part; e->td3_sums = sums; e->td3_gpart = gpart;
    e->td3_stored_t = e->ro_t;              // (days recorded before this call are not the trainer's)
    // theta starts as the device's policy; the targets as copies (of the critics too: zeros until they are uploaded and synchronised)
    td3_params_copy(e, kTd3Theta, 1);
    if ((rc = td3_sync_run(e))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_td3 = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_set_critic_layer(adc_engine *e, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    if (critic != 0 && critic != 1) return fail(ADC_EINVAL, "critic: 0 or 1");
    const adc::Td3Net &q = e->td3_shape.q;
    if (layer < 0 || layer >= q.layers) return fail(ADC_EINVAL, "no such critic layer");
    if (!weights_in_out || !bias_out) return fail(ADC_EINVAL, "weights or bias is NULL");
    ENGINE_GUARD(e);
    size_t off = (size_t)critic * (size_t)e->td3_Qc;
    for (int l = 0; l < layer; ++l) off += (size_t)(adc::td3_n_in(q, l) + 1) * (size_t)q.n_out[l];
    const size_t nw = (size_t)adc::td3_n_in(q, layer) * (size_t)q.n_out[layer];
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3Psi] + off, weights_in_out, nw * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3Psi] + off + nw, bias_out, (size_t)q.n_out[layer] * 4, hipMemcpyHostToDevice, e->stream));
    td3_params_copy(e, kTd3Psi, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_critic_set[critic][layer] = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_set_action_norm(adc_engine *e, const float *shift_a, const float *scale_a)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    if (!shift_a || !scale_a) return fail(ADC_EINVAL, "shift or scale is NULL");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->td3_a_shift, shift_a, (size_t)e->td3_shape.A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->td3_a_scale, scale_a, (size_t)e->td3_shape.A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_norm_set = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_sync_targets(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    ENGINE_GUARD(e);
    if (int rc = td3_sync_run(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_store(adc_engine *e, int64_t *stored)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = td3_ready(e)) || (rc = td3_state_check(e))) return rc;
    if (e->ro_t <= e->td3_stored_t) return fail(ADC_ESTATE, "no unstored day in the record (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    if (e->td3_gap || e->env_moves != e->ro_moves)
        return fail(ADC_ESTATE, "the envs were stepped or reset outside the record since an unstored recorded day: its next observation is not the "
                                "one the envs hold (adc_engine_rollout_reset, collect again)");
    ENGINE_GUARD(e);
    const long long count = (long long)(e->ro_t - e->td3_stored_t) * e->v.N;
    // (raw rows under a running observation normaliser: the last day's x' is the raw row an act would read now)
    hipLaunchKernelGGL(k_td3_store, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, e->tn.obs.count ? nullptr : e->mp.shift,
                       e->tn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A, e->ro_obs,
                       e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, (unsigned long long)e->td3_written,
                       (unsigned long long)e->td3_cfg.capacity);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_store_run(e, e->td3_written, count))) return rc;
    e->td3_written += count;
    e->td3_stored_t = e->ro_t;
    if (stored) *stored = count;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    if (size) *size = td3_size(e);
    if (written) *written = e->td3_written;
    if (capacity) *capacity = e->td3_cfg.capacity;
    return ADC_OK;
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
    if (slot < 0 || count < 1 || slot > td3_size(e) - count) return fail(ADC_EINVAL, "the slot range is not inside [0, size)");
    ENGINE_GUARD(e);
    const size_t s = (size_t)slot, n = (size_t)count, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
    const Td3Ring &g = e->td3_ring;
    if (x) HIP_TRY(hipMemcpyAsync(x, g.x + s * D, n * D * 4, hipMemcpyDeviceToHost, e->stream));
    if (a) HIP_TRY(hipMemcpyAsync(a, g.a + s * A, n * A * 4, hipMemcpyDeviceToHost, e->stream));
    if (r) HIP_TRY(hipMemcpyAsync(r, g.r + s, n * 4, hipMemcpyDeviceToHost, e->stream));
    if (done) HIP_TRY(hipMemcpyAsync(done, g.done + s, n, hipMemcpyDeviceToHost, e->stream));
    if (x2) HIP_TRY(hipMemcpyAsync(x2, g.x2 + s * D, n * D * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_buffer_load(adc_engine *e, int64_t slot, int64_t count, const float *x, const float *a, const float *r, const uint8_t *done,
                                          const float *x2, int64_t written)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    if (!x || !a || !r || !done || !x2) return fail(ADC_EINVAL, "x, a, r, done or x2 is NULL");
    if (slot < 0 || count < 1 || slot > (int64_t)e->td3_cfg.capacity - count) return fail(ADC_EINVAL, "the slot range is not inside [0, capacity)");
    if (written < slot + count) return fail(ADC_EINVAL, "written: at least slot + count");
    ENGINE_GUARD(e);
    const size_t s = (size_t)slot, n = (size_t)count, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
    const Td3Ring &g = e->td3_ring;
    HIP_TRY(hipMemcpyAsync(g.x + s * D, x, n * D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.a + s * A, a, n * A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.r + s, r, n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.done + s, done, n, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.x2 + s * D, x2, n * D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_written = written;
    if (e->per_live) {
        if (int rc = per_loaded_run(e, 0, slot, count)) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_batch_indices(adc_engine *e, int64_t update, int32_t *idx_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    if (!idx_b) return fail(ADC_EINVAL, "idx_b is NULL");
    if (update < 0 || update >= 0xFFFFFFFFll) return fail(ADC_EINVAL, "update: 0 to 2^32 - 2");
    if (td3_size(e) == 0) return fail(ADC_ESTATE, "the replay buffer is empty (adc_engine_td3_store)");
    if (e->per_live) return fail(ADC_ESTATE, "prioritised replay is alive on this engine: the batch is adc_engine_replay_prio_batch's, not the uniform law's");
    ENGINE_GUARD(e);
    const int B = e->td3_cfg.batch_size;
    hipLaunchKernelGGL(k_td3_indices, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, e->stream, e->td3_key, (uint32_t)update, (uint32_t)td3_size(e), B, e->td3_idx);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx_b, e->td3_idx, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_update(adc_engine *e, int32_t updates, adc_td3_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = td3_ready(e)) || (rc = td3_state_check(e))) return rc;
    if (updates < 1 || updates > 65536) return fail(ADC_EINVAL, "updates: 1 to 65536");
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < e->td3_shape.q.layers; ++l)
            if (!e->td3_critic_set[i][l]) return fail(ADC_ESTATE, "a critic layer has not been uploaded (adc_engine_td3_set_critic_layer)");
    if (td3_size(e) == 0) return fail(ADC_ESTATE, "the replay buffer is empty (adc_engine_td3_store)");
    if (e->td3_updates + updates >= 0xFFFFFFFFll) return fail(ADC_ESTATE, "the update counter is exhausted");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemsetAsync(e->td3_sums, 0, 16 * sizeof(double), e->stream));
    for (int i = 0; i < updates; ++i)
        // (the statistics' sums are taken for the call's last update and for its last actor step alone)
        if ((rc = td3_one_update(e, stats != nullptr, i + 1 == updates, updates - 1 - i < e->td3_cfg.policy_delay))) return rc;
    double sums[10] = {};
    if (stats) HIP_TRY(hipMemcpyAsync(sums, e->td3_sums, sizeof(sums), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) {
        const double n = (double)e->td3_cfg.batch_size;
        const double l1 = sums[adc::kTd3Loss1] / n, l2 = sums[adc::kTd3Loss2] / n, qpi = sums[8] / n;
        stats->updates = e->td3_updates; stats->actor_steps = e->td3_actor_steps; stats->buffer_size = td3_size(e); stats->samples = e->td3_cfg.batch_size;
        stats->critic_loss = l1 + l2;
        stats->q1_mean = sums[adc::kTd3Q1] / n; stats->q2_mean = sums[adc::kTd3Q2] / n; stats->y_mean = sums[adc::kTd3Y] / n;
        stats->actor_loss = -qpi;
        stats->critic_grad_norm = std::sqrt(sums[5]);
        stats->actor_grad_norm = std::sqrt(sums[9]);
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    if (actor_p) *actor_p = e->td3_P;
    if (critics_2qc) *critics_2qc = 2 * (int64_t)e->td3_Qc;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_state_get(adc_engine *e, float *theta_p, float *psi_q, float *theta_target_p, float *psi_target_q, float *m_theta_p,
                                        float *v_theta_p, float *m_psi_q, float *v_psi_q, int64_t *updates, int64_t *actor_steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    ENGINE_GUARD(e);
    const size_t pb = (size_t)e->td3_P * 4, qb = (size_t)e->td3_Qc * 8;
    float *flat[4] = {theta_p, psi_q, theta_target_p, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    for (int w = 0; w < 4; ++w) {
        if (flat[w]) HIP_TRY(hipMemcpyAsync(flat[w], e->td3_flat[w], (w & 1) ? qb : pb, hipMemcpyDeviceToHost, e->stream));
        if (mom[w]) HIP_TRY(hipMemcpyAsync(mom[w], e->td3_mom[w], w < 2 ? pb : qb, hipMemcpyDeviceToHost, e->stream));
    }
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
    if (int rc = td3_ready(e)) return rc;
    if (!theta_p || !psi_q || !theta_target_p || !psi_target_q || !m_theta_p || !v_theta_p || !m_psi_q || !v_psi_q) return fail(ADC_EINVAL, "a state vector is NULL");
    if (updates < 0 || updates >= 0x7FFFFFFFll || actor_steps < 0 || actor_steps > updates) return fail(ADC_EINVAL, "updates: 0 to 2^31 - 2; actor_steps: 0 to updates");
    ENGINE_GUARD(e);
    const size_t pb = (size_t)e->td3_P * 4, qb = (size_t)e->td3_Qc * 8;
    const float *flat[4] = {theta_p, psi_q, theta_target_p, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    for (int w = 0; w < 4; ++w) {
        HIP_TRY(hipMemcpyAsync(e->td3_flat[w], flat[w], (w & 1) ? qb : pb, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->td3_mom[w], mom[w], w < 2 ? pb : qb, hipMemcpyHostToDevice, e->stream));
        td3_params_copy(e, w, 0);           // (the device's policy layers, the critics and the targets follow the flat vectors)
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_updates = updates; e->td3_actor_steps = actor_steps;
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < e->td3_shape.q.layers; ++l) e->td3_critic_set[i][l] = true;
    return ADC_OK;
}
