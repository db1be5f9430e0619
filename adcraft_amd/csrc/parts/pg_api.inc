// pg_api.inc - the extern "C" entry points of policy-gradient training, of one learner and of a learner population (M PPO / A2C
// learners in lock-step, every launch over all members), over parts/pg_core.inc (include/adcraft_engine.h; the kernels are
// parts/kernel_pg.inc, the law csrc/adc_pg.h).  Everything here runs on the engine's own stream behind ENGINE_GUARD, that is after
// the env groups have joined: results do not depend on how the days were grouped.  One function serves both front ends; what
// differs in substance stays a visible branch: the single learner passes its loss constants, clip scale and step as kernel
// arguments and takes no upload, the population fills its member table on the host and uploads it once.
// (part of the single translation unit adc_engine.hip)
namespace {
// the law's chunked sum of `cols` columns of src into out[0 .. cols)
int pg_csum_launch(adc_engine *e, const float *src, long long n, int stride, int cols, int mode, double mean, double *out)
{
    const long long chunks = pg_chunks(n), lanes = chunks * cols;
    hipLaunchKernelGGL(k_pg_chunk_sums, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream, src, n, stride, cols, mode, mean, e->pg_part);
    hipLaunchKernelGGL(k_pg_join, dim3(1), dim3(64), 0, e->stream, e->pg_part, chunks, cols, out);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

adc::EsStep pg_step_of(const adc_pg_config &c, int64_t steps_taken)
{
    adc::EsStep step{};
    step.optimiser = c.optimiser == ADC_PG_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = c.lr; step.beta1 = c.beta1; step.beta2 = c.beta2; step.eps = c.eps; step.l2 = 0.0f;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(steps_taken + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(steps_taken + 1));
    return step;
}

// a member's constants from its configuration (what changes per call - moments, clip scale, step - is set where it is computed)
void pgp_member_fill(PgMember &m, const adc_pg_config &c)
{
    m.loss = adc::PgLoss{c.eps_clip, c.vf_coef, c.ent_coef};
    m.gamma = c.gamma; m.gl = c.gamma * c.lambda; m.reward_scale = c.reward_scale;
    m.normalize = c.normalize_advantages != 0;
}
int pgp_members_upload(adc_engine *e)
{
    HIP_TRY(hipMemcpyAsync(e->pgp_dmem, e->pgp_mem.data(), e->pgp_mem.size() * sizeof(PgMember), hipMemcpyHostToDevice, e->stream));
    return ADC_OK;
}
// the members' sums [M][16] in one copy
int pgp_sums_fetch(adc_engine *e)
{
    HIP_TRY(hipMemcpyAsync(e->pgp_host_sums.data(), e->pg_sums, e->pgp_host_sums.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
// every member's chunked sum of `cols` columns into pg_sums[member * 16 + at ...]
int pgp_csum_launch(adc_engine *e, const float *src, int n, int inner, int outer, size_t mstep, int stride, int cols, int mode, int at)
{
    const int chunks = (int)pg_chunks(n), lanes = chunks * cols, M = e->lrn_M;
    hipLaunchKernelGGL(k_pg_pop_chunk_sums, dim3((unsigned)((lanes + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, src, n, inner, outer, mstep, stride,
                       cols, mode, e->pgp_dmem, e->pg_part, e->pgp_part_stride);
    hipLaunchKernelGGL(k_pg_pop_join, dim3((unsigned)M), dim3(64), 0, e->stream, e->pg_part, e->pgp_part_stride, chunks, cols, e->pg_sums + at, 16);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

// GAE over the record under every member's constants, the advantages' normalisation where asked for, the start of an update
int pg_advantages_run(adc_engine *e)
{
    const bool pop = e->have_pg_pop;
    const int N = e->v.N, T = e->ro_t, M = pg_members(e), n = pg_member_envs(e);
    const long long tn = (long long)T * N;
    const dim3 grid((unsigned)((N + 255) / 256)), blk(256);
    int rc;
    if ((rc = pg_boot_launch(e))) return rc;
    // (rn.live: the reward times the running normaliser's multiplier - the env's, in a population - clipped: adc_rew_norm.h)
    if (pop) {
        if (e->rn.live)
            hipLaunchKernelGGL(k_rew_norm_pop_gae, grid, blk, 0, e->stream, N, T, n, e->pgp_dmem, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value, e->mlp_boot,
                               e->rn.rew.scale, N / e->rn.M, e->rn_cfg.clip, e->pg_adv, e->pg_ret);
        else
            hipLaunchKernelGGL(k_pg_pop_gae, grid, blk, 0, e->stream, N, T, n, e->pgp_dmem, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value, e->mlp_boot,
                               e->pg_adv, e->pg_ret);
    } else {
        const adc_pg_config &c = e->pgp_cfg[0];
        if (e->rn.live)
            hipLaunchKernelGGL(k_rew_norm_gae, grid, blk, 0, e->stream, N, T, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value, e->mlp_boot, c.gamma,
                               c.gamma * c.lambda, c.reward_scale, e->rn.rew.scale, e->rn_cfg.clip, e->pg_adv, e->pg_ret);
        else
            hipLaunchKernelGGL(k_pg_gae, grid, blk, 0, e->stream, N, T, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value, e->mlp_boot, c.gamma,
                               c.gamma * c.lambda, c.reward_scale, e->pg_adv, e->pg_ret);
    }
    HIP_TRY(hipGetLastError());
    bool any = !pop && e->pgp_cfg[0].normalize_advantages != 0;
    if (pop)
        for (const PgMember &m : e->pgp_mem) any = any || m.normalize;
    if (any && pop) {
        // the law's two passes per member over its T n samples in its own order i = t * n + local env; the moments finished on
        // the host as the single learner's are, all members' in one copy each way
        const int cnt = T * n;
        if ((rc = pgp_csum_launch(e, e->pg_adv, cnt, n, N, (size_t)n, 1, 1, 0, 0)) || (rc = pgp_sums_fetch(e))) return rc;
        for (int m = 0; m < M; ++m) e->pgp_mem[(size_t)m].mean = e->pgp_host_sums[(size_t)m * 16] / (double)cnt;
        if ((rc = pgp_members_upload(e)) || (rc = pgp_csum_launch(e, e->pg_adv, cnt, n, N, (size_t)n, 1, 1, 1, 0)) || (rc = pgp_sums_fetch(e))) return rc;
        for (int m = 0; m < M; ++m) e->pgp_mem[(size_t)m].sd = std::sqrt(e->pgp_host_sums[(size_t)m * 16] / (double)cnt);
        if ((rc = pgp_members_upload(e))) return rc;
        hipLaunchKernelGGL(k_pg_pop_normalize, dim3((unsigned)((tn + 255) / 256)), blk, 0, e->stream, e->pg_adv, tn, N, n, e->pgp_dmem);
        HIP_TRY(hipGetLastError());
    } else if (any) {
        double sum = 0.0, sq = 0.0;
        if ((rc = pg_csum_launch(e, e->pg_adv, tn, 1, 1, 0, 0.0, e->pg_sums))) return rc;
        HIP_TRY(hipMemcpyAsync(&sum, e->pg_sums, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const double mean = sum / (double)tn;
        if ((rc = pg_csum_launch(e, e->pg_adv, tn, 1, 1, 1, mean, e->pg_sums))) return rc;
        HIP_TRY(hipMemcpyAsync(&sq, e->pg_sums, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const double sd = std::sqrt(sq / (double)tn);
        hipLaunchKernelGGL(k_pg_normalize, dim3((unsigned)((tn + 255) / 256)), blk, 0, e->stream, e->pg_adv, tn, mean, sd);
        HIP_TRY(hipGetLastError());
    }
    if (e->kl_live)       // (the start of an update: the collecting distribution, adc_pg_kl.h)
        if ((rc = kl_snapshot_launch(e))) return rc;
    if (e->sh_live) sh_update_begin(e);
    e->pg_adv_ready = true;
    return ADC_OK;
}

// One gradient and one step of every member over the recorded days of its envs [n0, n0 + B) - or, g given (shuffled minibatches:
// adc_pg_shuffle.h), over its g->S samples whose record rows are g->rows + member * g->stride, with the early stop before the step.
// out_m: every member's statistics.  A population's member whose update has stopped is covered by the launches and left as it is
int pg_minibatch_run(adc_engine *e, int n0, int B, adc::PgStatsOut *out_m, const PgGather *g)
{
    const adc::PgShape &sh = e->pg_shape;
    const bool pop = e->have_pg_pop, kl = e->kl_live;
    const int N = e->v.N, M = pg_members(e), n = pg_member_envs(e), nd = adc::pg_deltas_floats(sh), Q = pg_Q(e);
    const long long S = g ? g->S : (long long)e->ro_t * B;
    const unsigned chunks = (unsigned)pg_chunks(S);
    if (!pop && g && e->sh_stats[0].stopped) {      // (the update has stopped: nothing to launch - the lock-step argument is the population's)
        e->sh_evaluated[0] = 0;
        if (out_m) *out_m = adc::PgStatsOut{};
        return ADC_OK;
    }
    const PgView p = pg_view_of(e, n0, B);
    const size_t lds = pg_lds_floats(sh, e->pg_maxw, kl) * sizeof(float);
    const dim3 sgrid((unsigned)S, (unsigned)M), blk(kPgBlock);
    if (pop) {
        if (g && kl) hipLaunchKernelGGL(k_pg_pop_gather_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), e->lrn_tab, e->pgp_dmem, e->kl_dmem, g->rows, g->stride);
        else if (g) hipLaunchKernelGGL(k_pg_pop_gather_sample, sgrid, blk, lds, e->stream, p, e->lrn_tab, e->pgp_dmem, g->rows, g->stride);
        else if (kl) hipLaunchKernelGGL(k_pg_pop_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), e->lrn_tab, e->pgp_dmem, e->kl_dmem, n);
        else hipLaunchKernelGGL(k_pg_pop_sample, sgrid, blk, lds, e->stream, p, e->lrn_tab, e->pgp_dmem, n);
    } else {
        const adc::PgKl klc = kl ? adc::PgKl{e->kl_coef[0], e->kl_cfg[0].vf_clip} : adc::PgKl{};
        if (g && kl) hipLaunchKernelGGL(k_pg_gather_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), klc, g->rows);
        else if (g) hipLaunchKernelGGL(k_pg_gather_sample, sgrid, blk, lds, e->stream, p, g->rows);
        else if (kl) hipLaunchKernelGGL(k_pg_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), klc);
        else hipLaunchKernelGGL(k_pg_sample, sgrid, blk, lds, e->stream, p);
    }
    pg_terms_walk(sh, e->ro_obs, e->pg_acts, p.na, [&](const PgTerm &t, unsigned tiles) {
        if (pop && g)
            hipLaunchKernelGGL(k_pg_pop_gather_wgrad, dim3(tiles, chunks, (unsigned)M), blk, 0, e->stream, t, S, g->rows, g->stride, e->pg_deltas, nd, e->pg_gpart, Q);
        else if (pop) hipLaunchKernelGGL(k_pg_pop_wgrad, dim3(tiles, chunks, (unsigned)M), blk, 0, e->stream, t, S, B, N, n0, n, e->pg_deltas, nd, e->pg_gpart, Q);
        else if (g) hipLaunchKernelGGL(k_pg_gather_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, g->rows, e->pg_deltas, nd, e->pg_gpart, Q);
        else hipLaunchKernelGGL(k_pg_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, B, N, n0, e->pg_deltas, nd, e->pg_gpart, Q);
    });
    if (pop) hipLaunchKernelGGL(k_pg_pop_grad_join, dim3(pg_blocks(Q), (unsigned)M), blk, 0, e->stream, e->pg_gpart, (int)chunks, Q, S, e->pg_grad);
    else hipLaunchKernelGGL(k_pg_grad_join, dim3(pg_blocks(Q)), blk, 0, e->stream, e->pg_gpart, (int)chunks, Q, S, e->pg_grad);
    HIP_TRY(hipGetLastError());
    int rc;
    if (!pop) {
        // the single learner: its sums on the stack, its clip scale and its step's constants kernel arguments
        if ((rc = pg_csum_launch(e, e->pg_pieces, S, adc::kPgPieces, 7, 0, 0.0, e->pg_sums)) ||
            (rc = pg_csum_launch(e, e->pg_pieces + adc::kPgRet, S, adc::kPgPieces, 2, 2, 0.0, e->pg_sums + 7)) ||
            (rc = pg_csum_launch(e, e->pg_grad, Q, 1, 1, 2, 0.0, e->pg_sums + 9)) ||
            (kl && (rc = pg_csum_launch(e, e->kl_pieces, S, adc::kPgKlPieces, adc::kPgKlPieces, 0, 0.0, e->pg_sums + adc::kPgSums))))
            return rc;
        double sums[adc::kPgSums + adc::kPgKlPieces];       // (the add-on's two sums are appended only while it lives)
        HIP_TRY(hipMemcpyAsync(sums, e->pg_sums, (size_t)(adc::kPgSums + (kl ? adc::kPgKlPieces : 0)) * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (kl) kl_stats_minibatch(e, 0, sums + adc::kPgSums, S);
        const adc_pg_config &c = e->pgp_cfg[0];
        const adc::PgStatsOut st = adc::pg_stats_finish(sums, S);
        if (out_m) *out_m = st;
        if (g && !sh_minibatch_evaluated(e, 0, st.approx_kl, S)) return ADC_OK;     // (stops here: no step, the count stays)
        const bool clip = c.max_grad_norm > 0.0f;
        const float scale = clip ? adc::pg_clip_scale(c.max_grad_norm, st.grad_norm) : 1.0f;
        hipLaunchKernelGGL(k_pg_update, dim3(pg_blocks(Q)), blk, 0, e->stream, e->pg_lay, e->pg_theta, e->pg_m, e->pg_v, e->pg_grad, clip ? 1 : 0, scale,
                           pg_step_of(c, e->pgp_steps[0]));
        HIP_TRY(hipGetLastError());
        e->pgp_steps[0] += 1;
        return ADC_OK;
    }
    if ((rc = pgp_csum_launch(e, e->pg_pieces, (int)S, 0, 0, (size_t)S, adc::kPgPieces, 7, 0, 0)) ||
        (rc = pgp_csum_launch(e, e->pg_pieces + adc::kPgRet, (int)S, 0, 0, (size_t)S, adc::kPgPieces, 2, 2, 7)) ||
        (rc = pgp_csum_launch(e, e->pg_grad, Q, 0, 0, (size_t)Q, 1, 1, 2, 9)) ||
        (kl && (rc = pgp_csum_launch(e, e->kl_pieces, (int)S, 0, 0, (size_t)S, adc::kPgKlPieces, adc::kPgKlPieces, 0, adc::kPgSums))) || (rc = pgp_sums_fetch(e)))
        return rc;
    // the population: the statistics, the clip scale and the step's constants of every member on the host, as the single learner's
    // are; up in one copy
    for (int m = 0; m < M; ++m) {
        const adc_pg_config &c = e->pgp_cfg[(size_t)m];
        PgMember &pm = e->pgp_mem[(size_t)m];
        const adc::PgStatsOut st = adc::pg_stats_finish(e->pgp_host_sums.data() + (size_t)m * 16, S);
        pm.clip = c.max_grad_norm > 0.0f;
        pm.scale = pm.clip ? adc::pg_clip_scale(c.max_grad_norm, st.grad_norm) : 1.0f;
        pm.step = pg_step_of(c, e->pgp_steps[(size_t)m]);
        const bool over = g && e->sh_stats[(size_t)m].stopped;     // (stopped before this minibatch: its statistics are none, as solo)
        if (out_m) out_m[m] = over ? adc::PgStatsOut{} : st;
        if (kl && !over) kl_stats_minibatch(e, m, e->pgp_host_sums.data() + (size_t)m * 16 + adc::kPgSums, S);
        if (g) pm.stopped = sh_minibatch_evaluated(e, m, st.approx_kl, S) ? 0 : 1;
    }
    if ((rc = pgp_members_upload(e))) return rc;
    if (g)
        hipLaunchKernelGGL(k_pg_pop_update_live, dim3(pg_blocks(Q), (unsigned)M), blk, 0, e->stream, e->lrn_lay, e->lrn_stride, e->pg_theta, e->pg_m, e->pg_v,
                           e->pg_grad, e->pgp_dmem);
    else
        hipLaunchKernelGGL(k_pg_pop_update, dim3(pg_blocks(Q), (unsigned)M), blk, 0, e->stream, e->lrn_lay, e->lrn_stride, e->pg_theta, e->pg_m, e->pg_v,
                           e->pg_grad, e->pgp_dmem);
    HIP_TRY(hipGetLastError());
    // (no wait here, as for the single learner: whoever writes the host's table next has waited for the stream since this upload -
    //  the sums' fetch of the next minibatch or normalisation pass, or adc_engine_pg_pop_set_config's own wait)
    for (int m = 0; m < M; ++m)
        if (!g || !e->pgp_mem[(size_t)m].stopped) e->pgp_steps[(size_t)m] += 1;
    return ADC_OK;
}

// adc_engine_pg_update / _pg_pop_update after the advantages, host-driven: per epoch the members' minibatches in env order, the
// statistics of the last epoch (under shuffled minibatches the loop is sh_update_run, parts/pg_shuffle_api.inc)
int pg_update_run(adc_engine *e, int epochs, adc_pg_stats *stats_m)
{
    const int M = pg_members(e), mb = e->pg_mb, count = pg_member_envs(e) / mb;
    std::vector<adc::PgStatsOut> o((size_t)M), acc((size_t)M), mean((size_t)M);
    KlEpoch kl;
    int rc;
    for (int ep = 0; ep < epochs; ++ep) {
        acc.assign((size_t)M, adc::PgStatsOut{});
        kl.begin(e);
        for (int i = 0; i < count; ++i) {
            if ((rc = pg_minibatch_run(e, i * mb, mb, o.data(), nullptr))) return rc;
            kl.add(e);
            for (size_t m = 0; m < (size_t)M; ++m) pg_stats_add(acc[m], o[m]);
        }
        for (size_t m = 0; m < (size_t)M; ++m) mean[m] = pg_stats_mean(acc[m], count);
    }
    if (e->kl_live && (rc = kl_update_end(e, kl))) return rc;       // (every member's adaptation: one small upload)
    if (stats_m)
        for (int m = 0; m < M; ++m) pg_stats_fill(stats_m + m, mean[(size_t)m], e->pgp_steps[(size_t)m], (int64_t)e->ro_t * mb);
    return ADC_OK;
}
int pg_advantages_enter(adc_engine *e, bool pop)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pg_enter(e, pop)) return rc;
    ENGINE_GUARD(e);
    return pg_advantages_run(e);
}
}  // namespace

ADC_EXPORT int adc_engine_pg_init(adc_engine *e, const adc_pg_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_pg_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    int rc;
    if ((rc = pg_state_check(e, false)) || (rc = pg_other_trainer_check(e))) return rc;
    const int N = e->v.N, mb = cfg->minibatch_envs == 0 ? N : cfg->minibatch_envs;
    if (mb > N || N % mb != 0) return fail(ADC_EINVAL, "minibatch_envs must divide num_envs");
    if (pg_chunks((long long)e->ro_T * mb) > 65535) return fail(ADC_EINVAL, "horizon x minibatch_envs: at most 65535 x 1024 samples in a minibatch");
    const adc::PgShape sh = adc::pg_shape_of(e->mlp_cfg, e->v.K, mlp_frames(e));
    const int maxw = pg_max_width(sh);
    if ((rc = pg_lds_refuse(e, sh, maxw, false))) return rc;
    ENGINE_GUARD(e);
    const PgLayout lay = centre_layout(e);      // the flat order against the device's stores
    const size_t Q = (size_t)lay.Q, tn = (size_t)e->ro_T * (size_t)N;
    if ((rc = pg_scratch_alloc(e, sh, maxw, 1, Q, mb, (size_t)pg_chunks((long long)std::max(tn, Q)) * 8u + 8u, false, cfg, 1))) return rc;
    e->pg_lay = lay;
    // theta starts as the device's weights
    hipLaunchKernelGGL(k_pg_params_copy, dim3(pg_blocks(lay.Q)), dim3(kPgBlock), 0, e->stream, lay, e->pg_theta, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_pg = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_init(adc_engine *e, const adc_pg_config *cfgs, int32_t count)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_state_check(e, true))) return rc;
    const int N = e->v.N, M = e->lrn_M, n = e->lrn_n;
    const char *why = nullptr;
    if (adc_pg_pop_config_check(cfgs, count, N, M, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if ((rc = pg_other_trainer_check(e))) return rc;
    if (e->have_pg) return fail(ADC_ESTATE, "a single-learner trainer is alive on this engine (adc_engine_pg_init)");
    const int mb = cfgs[0].minibatch_envs == 0 ? n : cfgs[0].minibatch_envs;
    if (pg_chunks((long long)e->ro_T * n) > 65535) return fail(ADC_EINVAL, "horizon x envs of a member: at most 65535 x 1024 samples");
    if (pg_chunks((long long)e->ro_T * mb) > 65535) return fail(ADC_EINVAL, "horizon x minibatch_envs: at most 65535 x 1024 samples in a minibatch");
    // (the member is the grid's y or z: adc_engine_mlp_learners admits at most 65535)
    const adc::PgShape sh = adc::pg_shape_of(e->mlp_cfg, e->v.K, mlp_frames(e));
    const int maxw = pg_max_width(sh);
    if ((rc = pg_lds_refuse(e, sh, maxw, false))) return rc;
    ENGINE_GUARD(e);
    const size_t Q = (size_t)e->lrn_lay.Q, Ms = (size_t)M;
    const size_t part_stride = (size_t)pg_chunks((long long)std::max((size_t)e->ro_T * (size_t)n, Q)) * 8u + 8u;
    if ((rc = pg_scratch_alloc(e, sh, maxw, Ms, Q, mb, part_stride, true, cfgs, count))) return rc;
    e->pgp_mem.assign(Ms, PgMember{});
    e->pgp_host_sums.assign(Ms * 16u, 0.0);
    for (size_t i = 0; i < Ms; ++i) pgp_member_fill(e->pgp_mem[i], e->pgp_cfg[i]);
    if ((rc = pgp_members_upload(e))) return rc;
    // every member's theta starts as its device weights
    hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks((int)Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, 0, e->pg_theta, Q, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_pg_pop = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_param_count(adc_engine *e, int64_t *count)
{
    if (!e || !count) return fail(ADC_EINVAL, "engine handle or count is NULL");
    if (int rc = pg_ready(e, false)) return rc;
    *count = e->pg_lay.Q;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_advantages(adc_engine *e) { return pg_advantages_enter(e, false); }
ADC_EXPORT int adc_engine_pg_pop_advantages(adc_engine *e) { return pg_advantages_enter(e, true); }
ADC_EXPORT int adc_engine_pg_advantages_fetch(adc_engine *e, float *adv_tn, float *ret_tn) { return pg_advantages_fetch(e, false, adv_tn, ret_tn); }
ADC_EXPORT int adc_engine_pg_pop_advantages_fetch(adc_engine *e, float *adv_tn, float *ret_tn) { return pg_advantages_fetch(e, true, adv_tn, ret_tn); }

ADC_EXPORT int adc_engine_pg_minibatch(adc_engine *e, int32_t env_begin, int32_t env_count, adc_pg_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_enter(e, false)) || (rc = pg_adv_check(e, false))) return rc;
    if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > e->v.N) return fail(ADC_EINVAL, "the env range is not inside [0, num_envs)");
    if (env_count > e->pg_mb) return fail(ADC_EINVAL, "env_count exceeds the configuration's minibatch_envs (the scratch was sized for it)");
    ENGINE_GUARD(e);
    adc::PgStatsOut o;
    if ((rc = pg_minibatch_run(e, env_begin, env_count, &o, nullptr))) return rc;
    if (stats) pg_stats_fill(stats, o, e->pgp_steps[0], (int64_t)e->ro_t * env_count);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_minibatch(adc_engine *e, int32_t index, adc_pg_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_enter(e, true)) || (rc = pg_adv_check(e, true))) return rc;
    if (index < 0 || index >= e->lrn_n / e->pg_mb) return fail(ADC_EINVAL, "no such minibatch: 0 to envs of a member / minibatch_envs - 1");
    ENGINE_GUARD(e);
    std::vector<adc::PgStatsOut> o((size_t)e->lrn_M);
    if ((rc = pg_minibatch_run(e, index * e->pg_mb, e->pg_mb, o.data(), nullptr))) return rc;
    if (stats_m)
        for (int m = 0; m < e->lrn_M; ++m) pg_stats_fill(stats_m + m, o[(size_t)m], e->pgp_steps[(size_t)m], (int64_t)e->ro_t * e->pg_mb);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_state_get(adc_engine *e, float *theta_q, float *m_q, float *v_q, int64_t *steps)
{
    return pg_state_get(e, false, 0, theta_q, m_q, v_q, steps);
}
ADC_EXPORT int adc_engine_pg_state_set(adc_engine *e, const float *theta_q, const float *m_q, const float *v_q, int64_t steps)
{
    return pg_state_set(e, false, 0, theta_q, m_q, v_q, steps);
}
ADC_EXPORT int adc_engine_pg_pop_state_get(adc_engine *e, int32_t member, float *theta_q, float *m_q, float *v_q, int64_t *steps)
{
    return pg_state_get(e, true, member, theta_q, m_q, v_q, steps);
}
ADC_EXPORT int adc_engine_pg_pop_state_set(adc_engine *e, int32_t member, const float *theta_q, const float *m_q, const float *v_q, int64_t steps)
{
    return pg_state_set(e, true, member, theta_q, m_q, v_q, steps);
}

ADC_EXPORT int adc_engine_pg_pop_set_config(adc_engine *e, int32_t member, const adc_pg_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e, true)) || (rc = pg_member_check(e, member))) return rc;
    const char *why = nullptr;
    if (adc_pg_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if ((cfg->minibatch_envs == 0 ? e->lrn_n : cfg->minibatch_envs) != e->pg_mb)
        return fail(ADC_EINVAL, "minibatch_envs may not change: the members' minibatches run in the same launches (the scratch was sized for it)");
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));       // (an upload of the host's table may still be in flight)
    e->pgp_cfg[(size_t)member] = *cfg;
    pgp_member_fill(e->pgp_mem[(size_t)member], *cfg);
    if ((rc = pgp_members_upload(e))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pg_adv_ready = false;            // (advantages computed under the old gamma, lambda, reward_scale or normalisation are stale)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_copy(adc_engine *e, int32_t src, int32_t dst)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e, true)) || (rc = pg_member_check(e, src)) || (rc = pg_member_check(e, dst))) return rc;
    if (src == dst) return ADC_OK;
    ENGINE_GUARD(e);
    const size_t Q = (size_t)e->lrn_lay.Q, bytes = Q * 4, from = (size_t)src * Q, to = (size_t)dst * Q;
    HIP_TRY(hipMemcpyAsync(e->pg_theta + to, e->pg_theta + from, bytes, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_m + to, e->pg_m + from, bytes, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_v + to, e->pg_v + from, bytes, hipMemcpyDeviceToDevice, e->stream));
    if ((rc = pg_params_follow(e, dst))) return rc;
    e->pgp_steps[(size_t)dst] = e->pgp_steps[(size_t)src];
    return kl_copy(e, 1, [&](int, int &d, int &f) { d = dst; f = src; });      // (the donor's KL coefficient)
}

// ---- the queued update: a whole update enqueued as one chain, one wait (include/adcraft_engine.h; parts/kernel_pg_queued.inc) --------
// After the advantages nothing of an update needs the host but two decisions per step - the target-KL stop and the norm clip's scale -
// and k_pg_decide takes them on the device by the host's law (adc_pg_shuffle.h: pg_decide).  What the host-driven update learns
// step by step is known in advance or not needed until the end: a member that has not stopped has taken s0 + epoch * minibatches
// steps when an epoch begins, so every epoch's tick is host-known (a stopped member's order is never read); the step's constants
// are a table over the steps s0 ... s0 + epochs * minibatches - 1, indexed on the device by the steps the member has taken; the
// statistics are finished after the one wait from the log of raw sums, by the code of the host-driven loops.
namespace {
// the sections of the device block (and of its pinned twin), byte offsets: [0, ctl) goes up in one copy, [ctl, end) comes down in one
struct PqPlan {
    int M, epochs, count, cap;          // members; epochs; minibatches of an epoch; minibatches of the update = rows of a member's step table
    size_t law, steps, ticks, ctl, log, end;
};
inline size_t pq_up16(size_t x) { return (x + 15u) & ~(size_t)15u; }
PqPlan pq_plan(int M, int epochs, int count, bool shuffle)
{
    PqPlan p{};
    p.M = M; p.epochs = epochs; p.count = count; p.cap = epochs * count;
    const size_t Ms = (size_t)M, cap = (size_t)p.cap;
    size_t at = 0;
    p.law = at; at = pq_up16(at + Ms * sizeof(PgQLaw));
    p.steps = at; at = pq_up16(at + Ms * cap * sizeof(adc::EsStep));
    p.ticks = at; at = pq_up16(at + (shuffle ? (size_t)epochs * Ms * sizeof(PgShuffleMember) : 0u));
    p.ctl = at; at = pq_up16(at + Ms * sizeof(PgQCtl));
    p.log = at; at += cap * Ms * sizeof(PgQRow);
    p.end = at;
    return p;
}
// the block and its twin hold `bytes` (the new pair is allocated before the old one goes: a refusal leaves the engine as it was)
int pq_reserve(adc_engine *e, size_t bytes)
{
    if (bytes <= e->pq_bytes) return ADC_OK;
    std::vector<void *> fresh;
    uint8_t *dev = nullptr;
    void *host = nullptr;
    if (int rc = mlp_alloc(e, fresh, &dev, bytes)) { mlp_free(e, fresh); return rc; }
    if (hipHostMalloc(&host, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        mlp_free(e, fresh);
        return fail(ADC_ENOMEM, "hipHostMalloc failed (the queued update's log)");
    }
    if (const hipError_t err = hipStreamSynchronize(e->stream); err != hipSuccess) {       // (nothing old has gone yet)
        mlp_free(e, fresh);
        (void)hipHostFree(host);
        return fail(ADC_EHIP, std::string("hipStreamSynchronize(e->stream): ") + hipGetErrorString(err));
    }
    sh_replace(e, e->pq_dev, dev);
    e->pg_allocs.push_back(dev);
    if (e->pq_host) (void)hipHostFree(e->pq_host);
    e->pq_host = static_cast<uint8_t *>(host);
    e->pq_bytes = bytes;
    return ADC_OK;
}
// a member's step table: pg_step_of(c, s0 + i) for i < cap.  es_bias_correction's product beta^t is t products from 1 in order, so
// the next row's is this row's times beta - the same chain, the same bits, without walking it from 1 for every row
void pq_steps_fill(adc::EsStep *out, const adc_pg_config &c, int64_t s0, int cap)
{
    adc::EsStep step = pg_step_of(c, s0);
    double p1 = 1.0, p2 = 1.0;
    for (uint32_t k = 0, t = (uint32_t)(s0 + 1); k < t; ++k) { p1 = p1 * (double)step.beta1; p2 = p2 * (double)step.beta2; }
    for (int i = 0; i < cap; ++i) {
        step.c1 = (float)(1.0 - p1); step.c2 = (float)(1.0 - p2);
        out[i] = step;
        p1 = p1 * (double)step.beta1; p2 = p2 * (double)step.beta2;
    }
}

// pg_minibatch_run without the host in the middle: minibatch `index` of an epoch (g given: the gathered one) of
// every member, its decision and its step enqueued; row `serial` of the log takes its sums
int pq_minibatch_enqueue(adc_engine *e, const PqPlan &pl, int index, int serial, const PgGather *g)
{
    const adc::PgShape &sh = e->pg_shape;
    const bool pop = e->have_pg_pop, kl = e->kl_live;
    const int N = e->v.N, M = pl.M, n = pg_member_envs(e), B = g ? 1 : e->pg_mb, n0 = g ? 0 : index * B, nd = adc::pg_deltas_floats(sh), Q = pg_Q(e);
    const long long S = g ? g->S : (long long)e->ro_t * B;
    const unsigned chunks = (unsigned)pg_chunks(S);
    const PgQCtl *ctl = reinterpret_cast<const PgQCtl *>(e->pq_dev + pl.ctl);
    const PgView p = pg_view_of(e, n0, B);
    const size_t lds = pg_lds_floats(sh, e->pg_maxw, kl) * sizeof(float);
    const dim3 sgrid((unsigned)S, (unsigned)M), blk(kPgBlock);
    if (pop) {
        if (g && kl)
            hipLaunchKernelGGL(k_pg_pop_q_gather_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), e->lrn_tab, e->pgp_dmem, e->kl_dmem, g->rows, g->stride, ctl);
        else if (g)
            hipLaunchKernelGGL(k_pg_pop_q_gather_sample, sgrid, blk, lds, e->stream, p, e->lrn_tab, e->pgp_dmem, g->rows, g->stride, ctl);
        else if (kl)
            hipLaunchKernelGGL(k_pg_pop_q_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), e->lrn_tab, e->pgp_dmem, e->kl_dmem, n, ctl);
        else
            hipLaunchKernelGGL(k_pg_pop_q_sample, sgrid, blk, lds, e->stream, p, e->lrn_tab, e->pgp_dmem, n, ctl);
    } else {
        const adc::PgKl klc = kl ? adc::PgKl{e->kl_coef[0], e->kl_cfg[0].vf_clip} : adc::PgKl{};
        if (g && kl) hipLaunchKernelGGL(k_pg_q_gather_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), klc, g->rows, ctl);
        else if (g) hipLaunchKernelGGL(k_pg_q_gather_sample, sgrid, blk, lds, e->stream, p, g->rows, ctl);
        else if (kl) hipLaunchKernelGGL(k_pg_q_kl_sample, sgrid, blk, lds, e->stream, p, kl_view(e), klc, ctl);
        else hipLaunchKernelGGL(k_pg_q_sample, sgrid, blk, lds, e->stream, p, ctl);
    }
    pg_terms_walk(sh, e->ro_obs, e->pg_acts, p.na, [&](const PgTerm &t, unsigned tiles) {
        if (pop && g)
            hipLaunchKernelGGL(k_pg_pop_q_gather_wgrad, dim3(tiles, chunks, (unsigned)M), blk, 0, e->stream, t, S, g->rows, g->stride, e->pg_deltas, nd,
                               e->pg_gpart, Q, ctl);
        else if (pop)
            hipLaunchKernelGGL(k_pg_pop_q_wgrad, dim3(tiles, chunks, (unsigned)M), blk, 0, e->stream, t, S, B, N, n0, n, e->pg_deltas, nd, e->pg_gpart, Q, ctl);
        else if (g)
            hipLaunchKernelGGL(k_pg_q_gather_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, g->rows, e->pg_deltas, nd, e->pg_gpart, Q, ctl);
        else
            hipLaunchKernelGGL(k_pg_q_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, B, N, n0, e->pg_deltas, nd, e->pg_gpart, Q, ctl);
    });
    hipLaunchKernelGGL(k_pg_q_grad_join, dim3(pg_blocks(Q), (unsigned)M), blk, 0, e->stream, e->pg_gpart, (int)chunks, Q, S, e->pg_grad, ctl);
    // the statistics' sums of every member into pg_sums[member * 16 + at ...], as pgp_csum_launch / pg_csum_launch order them
    const size_t part_stride = pop ? e->pgp_part_stride : (size_t)0;
    auto csum = [&](const float *src, int cnt, int stride, int cols, int mode, int at) {
        const int ch = (int)pg_chunks(cnt), lanes = ch * cols;
        hipLaunchKernelGGL(k_pg_q_chunk_sums, dim3((unsigned)((lanes + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, src, cnt, (size_t)cnt, stride, cols,
                           mode, e->pg_part, part_stride, ctl);
        hipLaunchKernelGGL(k_pg_q_join, dim3((unsigned)M), dim3(64), 0, e->stream, e->pg_part, part_stride, ch, cols, e->pg_sums + at, 16, ctl);
    };
    csum(e->pg_pieces, (int)S, adc::kPgPieces, 7, 0, 0);
    csum(e->pg_pieces + adc::kPgRet, (int)S, adc::kPgPieces, 2, 2, 7);
    csum(e->pg_grad, Q, 1, 1, 2, 9);
    if (kl) csum(e->kl_pieces, (int)S, adc::kPgKlPieces, adc::kPgKlPieces, 0, adc::kPgSums);
    hipLaunchKernelGGL(k_pg_decide, dim3((unsigned)M), dim3(kWave), 0, e->stream, e->pg_sums, adc::kPgSums + (kl ? adc::kPgKlPieces : 0), (int)S, g ? 1 : 0,
                       reinterpret_cast<const PgQLaw *>(e->pq_dev + pl.law), reinterpret_cast<PgQCtl *>(e->pq_dev + pl.ctl),
                       reinterpret_cast<PgQRow *>(e->pq_dev + pl.log) + (size_t)serial * (size_t)M);
    const adc::EsStep *steps = reinterpret_cast<const adc::EsStep *>(e->pq_dev + pl.steps);
    if (pop)
        hipLaunchKernelGGL(k_pg_pop_q_update, dim3(pg_blocks(Q), (unsigned)M), blk, 0, e->stream, e->lrn_lay, e->lrn_stride, e->pg_theta, e->pg_m, e->pg_v,
                           e->pg_grad, ctl, steps, pl.cap);
    else
        hipLaunchKernelGGL(k_pg_q_update, dim3(pg_blocks(Q)), blk, 0, e->stream, e->pg_lay, e->pg_theta, e->pg_m, e->pg_v, e->pg_grad, ctl, steps);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

// adc_engine_pg_update_queued / _pg_pop_update_queued after the advantages
int pq_update_run(adc_engine *e, int epochs, adc_pg_stats *stats_m)
{
    const bool pop = e->have_pg_pop, shuffle = e->sh_live, kl = e->kl_live;
    const int M = pg_members(e), n = pg_member_envs(e), N = e->v.N;
    const uint32_t n_s = (uint32_t)e->ro_t * (uint32_t)n;
    if (shuffle) e->sh_ns = n_s;
    const int count = shuffle ? sh_minibatches(e) : n / e->pg_mb;
    if ((long long)epochs * count > (1ll << 22)) return fail(ADC_EINVAL, "epochs x minibatches: at most 2^22 steps in one queued update (its log and step tables)");
    const PqPlan pl = pq_plan(M, epochs, count, shuffle);
    int rc;
    if ((rc = pq_reserve(e, pl.end))) return rc;
    // 2. the tables, up once
    std::memset(e->pq_host, 0, pl.log);
    PgQLaw *law = reinterpret_cast<PgQLaw *>(e->pq_host + pl.law);
    adc::EsStep *steps = reinterpret_cast<adc::EsStep *>(e->pq_host + pl.steps);
    PgShuffleMember *ticks = reinterpret_cast<PgShuffleMember *>(e->pq_host + pl.ticks);
    for (int m = 0; m < M; ++m) {
        const adc_pg_config &c = e->pgp_cfg[(size_t)m];
        law[m] = PgQLaw{c.max_grad_norm, shuffle ? e->sh_cfg[(size_t)m].target_kl : 0.0f};
        pq_steps_fill(steps + (size_t)m * (size_t)pl.cap, c, e->pgp_steps[(size_t)m], pl.cap);
        if (shuffle)
            for (int ep = 0; ep < epochs; ++ep) {       // (a live member has taken exactly ep * count steps of this update when epoch ep begins)
                PgShuffleMember &t = ticks[(size_t)ep * (size_t)M + (size_t)m];
                t.key = e->sh_mem[(size_t)m].key;
                t.tick = (uint32_t)((uint64_t)(e->pgp_steps[(size_t)m] + (int64_t)ep * count) & 0xFFFFFFFFull);
            }
    }
    HIP_TRY(hipMemcpyAsync(e->pq_dev, e->pq_host, pl.log, hipMemcpyHostToDevice, e->stream));
    if (pop && (rc = pgp_members_upload(e))) return rc;
    // 3. every epoch's order and every minibatch's kernels, no wait
    for (int ep = 0; ep < epochs; ++ep) {
        if (shuffle) {
            hipLaunchKernelGGL(k_pg_shuffle_rows, dim3((n_s + 255u) / 256u, (unsigned)M), dim3(256), 0, e->stream,
                               reinterpret_cast<const PgShuffleMember *>(e->pq_dev + pl.ticks) + (size_t)ep * (size_t)M, n_s, adc::pg_shuffle_half_bits(n_s),
                               (uint32_t)n, (uint32_t)N, e->sh_order, e->sh_rows);
            HIP_TRY(hipGetLastError());
        }
        for (int j = 0; j < count; ++j) {
            const PgGather g = shuffle ? sh_gather(e, j) : PgGather{};
            if ((rc = pq_minibatch_enqueue(e, pl, j, ep * count + j, shuffle ? &g : nullptr))) return rc;
        }
    }
    // 4., 5. the control blocks and the log down in one copy, the one wait
    HIP_TRY(hipMemcpyAsync(e->pq_host + pl.ctl, e->pq_dev + pl.ctl, pl.end - pl.ctl, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // the host-driven loops over the log: adc_engine_pg_update's / _pg_pop_update's, or sh_update_run's under shuffled minibatches
    const PgQCtl *ctl = reinterpret_cast<const PgQCtl *>(e->pq_host + pl.ctl);
    const PgQRow *log = reinterpret_cast<const PgQRow *>(e->pq_host + pl.log);
    std::vector<adc::PgStatsOut> acc((size_t)M), mean((size_t)M);
    std::vector<int> cnt((size_t)M, 0);
    std::vector<int64_t> taken((size_t)M, 0);
    std::vector<uint8_t> live((size_t)M, 1);
    KlEpoch klep;
    bool agree = true;
    if (!shuffle) {
        for (int ep = 0; ep < epochs; ++ep) {
            acc.assign((size_t)M, adc::PgStatsOut{});
            klep.begin(e);
            for (int j = 0; j < count; ++j) {
                for (int m = 0; m < M; ++m) {
                    const PgQRow &r = log[((size_t)ep * (size_t)count + (size_t)j) * (size_t)M + (size_t)m];
                    agree = agree && r.evaluated == 1;
                    if (kl) kl_stats_minibatch(e, m, r.sums + adc::kPgSums, r.count);
                    pg_stats_add(acc[(size_t)m], adc::pg_stats_finish(r.sums, r.count));
                    taken[(size_t)m] += 1;
                }
                klep.add(e);
            }
            for (int m = 0; m < M; ++m) mean[(size_t)m] = pg_stats_mean(acc[(size_t)m], count);
        }
    } else {
        for (int ep = 0; ep < epochs && !sh_all_stopped(e); ++ep) {
            for (int m = 0; m < M; ++m) {
                live[(size_t)m] = !e->sh_stats[(size_t)m].stopped;
                if (live[(size_t)m]) { e->sh_stats[(size_t)m].epochs_begun += 1; acc[(size_t)m] = adc::PgStatsOut{}; cnt[(size_t)m] = 0; }
            }
            klep.begin(e, live.data());
            for (int j = 0; j < count && !sh_all_stopped(e); ++j) {
                for (int m = 0; m < M; ++m) {
                    const PgQRow &r = log[((size_t)ep * (size_t)count + (size_t)j) * (size_t)M + (size_t)m];
                    const bool over = e->sh_stats[(size_t)m].stopped != 0;
                    agree = agree && (r.evaluated != 0) == !over;
                    if (over) { e->sh_evaluated[(size_t)m] = 0; continue; }
                    if (kl) kl_stats_minibatch(e, m, r.sums + adc::kPgSums, r.count);
                    const adc::PgStatsOut st = adc::pg_stats_finish(r.sums, r.count);
                    if (sh_minibatch_evaluated(e, m, st.approx_kl, r.count)) taken[(size_t)m] += 1;
                    pg_stats_add(acc[(size_t)m], st);
                    cnt[(size_t)m] += 1;
                }
                klep.add(e, e->sh_evaluated.data());
            }
            for (int m = 0; m < M; ++m)
                if (live[(size_t)m]) mean[(size_t)m] = pg_stats_mean(acc[(size_t)m], cnt[(size_t)m]);
        }
        e->sh_epoch_ready = false;      // (the chain drew every epoch's order over the last one's: none of them is kept for a later call)
    }
    for (int m = 0; m < M; ++m) {
        agree = agree && ctl[m].taken == taken[(size_t)m] && (ctl[m].stopped != 0) == (shuffle && e->sh_stats[(size_t)m].stopped);
        e->pgp_steps[(size_t)m] += taken[(size_t)m];
    }
    // (one law, two sides: a difference would mean the device took steps the host's statistics do not describe - never silently)
    if (!agree) return fail(ADC_EHIP, "the queued update's device decisions and their replay on the host disagree");
    if (kl && (rc = kl_update_end(e, klep, true))) return rc;
    if (stats_m)
        for (int m = 0; m < M; ++m)
            pg_stats_fill(stats_m + m, mean[(size_t)m], e->pgp_steps[(size_t)m], shuffle ? e->sh_last_count[(size_t)m] : (int64_t)e->ro_t * e->pg_mb);
    return ADC_OK;
}
// the three updates' entry: the preamble, the advantages, then the loop that was asked for
int pg_update_enter(adc_engine *e, bool pop, int32_t epochs, adc_pg_stats *stats_m, bool queued)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_enter(e, pop, epochs))) return rc;
    ENGINE_GUARD(e);
    if ((rc = pg_advantages_run(e))) return rc;
    if (queued) return pq_update_run(e, epochs, stats_m);
    return e->sh_live ? sh_update_run(e, epochs, stats_m) : pg_update_run(e, epochs, stats_m);
}
}  // namespace

ADC_EXPORT int adc_engine_pg_update(adc_engine *e, int32_t epochs, adc_pg_stats *stats) { return pg_update_enter(e, false, epochs, stats, false); }
ADC_EXPORT int adc_engine_pg_pop_update(adc_engine *e, int32_t epochs, adc_pg_stats *stats_m) { return pg_update_enter(e, true, epochs, stats_m, false); }
ADC_EXPORT int adc_engine_pg_update_queued(adc_engine *e, int32_t epochs, adc_pg_stats *stats) { return pg_update_enter(e, false, epochs, stats, true); }
ADC_EXPORT int adc_engine_pg_pop_update_queued(adc_engine *e, int32_t epochs, adc_pg_stats *stats_m) { return pg_update_enter(e, true, epochs, stats_m, true); }
