// pg_api.inc - the extern "C" entry points of policy-gradient training (include/adcraft_engine.h; the kernels are
// parts/kernel_pg.inc, the law csrc/adc_pg.h).  Everything here runs on the engine's own stream behind ENGINE_GUARD, that is
// after the env groups have joined: results do not depend on how the days were grouped.
// (part of the single translation unit adc_engine.hip)
namespace {
int pg_ready(const adc_engine *e)
{
    if (!e->have_pg) return fail(ADC_ESTATE, "adc_engine_pg_init has not been called (or the policy / the record was re-initialised since)");
    return ADC_OK;
}
// what a policy-gradient call needs of the engine's state, checked at init and again at every call
int pg_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (e->pop_M != 0) return fail(ADC_ESTATE, "policy-gradient training with a population active is not supported (adc_engine_mlp_population(0) first)");
    if (e->lrn_M != 0) return fail(ADC_ESTATE, "learners are active: they train through adc_engine_pg_pop_init (adc_engine_mlp_learners(0) first)");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "policy-gradient training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "policy-gradient training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
int pg_record_check(const adc_engine *e)
{
    if (e->ro_t == 0) return fail(ADC_ESTATE, "no day has been recorded (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    if (e->ro_deterministic)
        return fail(ADC_ESTATE, "the record holds days collected with the deterministic policy: their log-probabilities mean nothing "
                                "(adc_engine_mlp_set_deterministic(0), adc_engine_rollout_reset, collect again)");
    return ADC_OK;
}
inline long long pg_chunks(long long n) { return (n + adc::kPgChunk - 1) / adc::kPgChunk; }

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

int pg_advantages_run(adc_engine *e)
{
    const int N = e->v.N, T = e->ro_t;
    const long long n = (long long)T * N;
    if (e->mp.val.layers > 0)
        mlp_launch_kernel(e->v, e->mp, e->stream, 1, nullptr, 0.0f, e->d_bids, e->d_budget, MlpRecordSlot{nullptr, nullptr, nullptr, nullptr}, e->mlp_boot);
    else HIP_TRY(hipMemsetAsync(e->mlp_boot, 0, (size_t)N * 4, e->stream));
    const adc_pg_config &c = e->pg_cfg;
    if (e->rn.live)       // (the reward times the running normaliser's multiplier, clipped: adc_rew_norm.h)
        hipLaunchKernelGGL(k_rew_norm_gae, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, N, T, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value,
                           e->mlp_boot, c.gamma, c.gamma * c.lambda, c.reward_scale, e->rn.rew.scale, e->rn_cfg.clip, e->pg_adv, e->pg_ret);
    else
        hipLaunchKernelGGL(k_pg_gae, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, N, T, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value,
                           e->mlp_boot, c.gamma, c.gamma * c.lambda, c.reward_scale, e->pg_adv, e->pg_ret);
    HIP_TRY(hipGetLastError());
    if (c.normalize_advantages) {
        double sum = 0.0, sq = 0.0;
        if (int rc = pg_csum_launch(e, e->pg_adv, n, 1, 1, 0, 0.0, e->pg_sums)) return rc;
        HIP_TRY(hipMemcpyAsync(&sum, e->pg_sums, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const double mean = sum / (double)n;
        if (int rc = pg_csum_launch(e, e->pg_adv, n, 1, 1, 1, mean, e->pg_sums)) return rc;
        HIP_TRY(hipMemcpyAsync(&sq, e->pg_sums, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const double sd = std::sqrt(sq / (double)n);
        hipLaunchKernelGGL(k_pg_normalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->pg_adv, n, mean, sd);
        HIP_TRY(hipGetLastError());
    }
    if (e->kl_live)       // (the start of an update: the collecting distribution, adc_pg_kl.h)
        if (int rc = kl_snapshot_launch(e)) return rc;
    if (e->sh_live) sh_update_begin(e);
    e->pg_adv_ready = true;
    return ADC_OK;
}

// one gradient and one step over the recorded days of the envs [n0, n0 + B) - or, g given (shuffled minibatches: adc_pg_shuffle.h),
// over the g->S samples whose record rows are g->rows, with the early stop before the step
int pg_minibatch_run(adc_engine *e, int n0, int B, adc::PgStatsOut *out, const PgGather *g)
{
    const adc::PgShape &sh = e->pg_shape;
    const int N = e->v.N, T = e->ro_t, na = adc::pg_acts_floats(sh), nd = adc::pg_deltas_floats(sh);
    const long long S = g ? g->S : (long long)T * B;
    if (g && e->sh_stats[0].stopped) {      // (the update has stopped: nothing to launch - the lock-step argument is the population's)
        e->sh_evaluated[0] = 0;
        if (out) *out = adc::PgStatsOut{};
        return ADC_OK;
    }
    PgView p{};
    p.sh = sh;
    p.loss = adc::PgLoss{e->pg_cfg.eps_clip, e->pg_cfg.vf_coef, e->pg_cfg.ent_coef};
    p.net[0] = e->mp.pol; p.net[1] = e->mp.val;
    p.log_std = e->mp.log_std;
    p.obs = e->ro_obs; p.action = e->ro_action; p.logp = e->ro_logp; p.value = e->ro_value;
    p.adv = e->pg_adv; p.ret = e->pg_ret;
    p.N = N; p.n0 = n0; p.B = B;
    p.acts = e->pg_acts; p.deltas = e->pg_deltas; p.pieces = e->pg_pieces;
    p.na = na; p.nd = nd; p.maxw = e->pg_maxw;
    const bool kl = e->kl_live;
    if (g && kl)
        hipLaunchKernelGGL(k_pg_gather_kl_sample, dim3((unsigned)S), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw, true) * sizeof(float), e->stream, p,
                           kl_view(e), adc::PgKl{e->kl_coef[0], e->kl_cfg[0].vf_clip}, g->rows);
    else if (g)
        hipLaunchKernelGGL(k_pg_gather_sample, dim3((unsigned)S), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw) * sizeof(float), e->stream, p, g->rows);
    else if (kl)
        hipLaunchKernelGGL(k_pg_kl_sample, dim3((unsigned)S), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw, true) * sizeof(float), e->stream, p, kl_view(e),
                           adc::PgKl{e->kl_coef[0], e->kl_cfg[0].vf_clip});
    else
        hipLaunchKernelGGL(k_pg_sample, dim3((unsigned)S), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw) * sizeof(float), e->stream, p);
    // the gradient's terms in the flat order
    {
        int flat = 0, ao = 0, dof = 0;
        auto launch = [&](const float *X, size_t ldx, int n_in, int n_out, int obs) {
            PgTerm t{X, ldx, n_in, n_out, dof, flat, obs};
            const unsigned tiles = (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile));
            if (g)
                hipLaunchKernelGGL(k_pg_gather_wgrad, dim3(tiles, (unsigned)pg_chunks(S)), dim3(kPgBlock), 0, e->stream, t, S, g->rows, e->pg_deltas, nd,
                                   e->pg_gpart, e->pg_lay.Q);
            else
                hipLaunchKernelGGL(k_pg_wgrad, dim3(tiles, (unsigned)pg_chunks(S)), dim3(kPgBlock), 0, e->stream, t, S, B, N, n0, e->pg_deltas, nd,
                                   e->pg_gpart, e->pg_lay.Q);
            flat += (n_in + 1) * n_out;
        };
        for (int net = 0; net < 2; ++net)
            for (int l = 0; l < sh.layers[net]; ++l) {
                const int n_in = adc::pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
                if (l == 0) launch(e->ro_obs, (size_t)sh.D, n_in, n_out, 1);
                else { launch(e->pg_acts + ao, (size_t)na, n_in, n_out, 0); ao += n_in; }
                dof += n_out;
            }
        if (!sh.two_heads) launch(nullptr, 0, 0, sh.A, 0);
    }
    const int Q = e->pg_lay.Q;
    hipLaunchKernelGGL(k_pg_grad_join, dim3((unsigned)((Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->pg_gpart, (int)pg_chunks(S), Q, S,
                       e->pg_grad);
    HIP_TRY(hipGetLastError());
    int rc;
    if ((rc = pg_csum_launch(e, e->pg_pieces, S, adc::kPgPieces, 7, 0, 0.0, e->pg_sums)) ||
        (rc = pg_csum_launch(e, e->pg_pieces + adc::kPgRet, S, adc::kPgPieces, 2, 2, 0.0, e->pg_sums + 7)) ||
        (rc = pg_csum_launch(e, e->pg_grad, Q, 1, 1, 2, 0.0, e->pg_sums + 9)) ||
        (kl && (rc = pg_csum_launch(e, e->kl_pieces, S, adc::kPgKlPieces, adc::kPgKlPieces, 0, 0.0, e->pg_sums + adc::kPgSums))))
        return rc;
    double sums[adc::kPgSums + adc::kPgKlPieces];       // (the add-on's two sums are appended only while it lives)
    HIP_TRY(hipMemcpyAsync(sums, e->pg_sums, (size_t)(adc::kPgSums + (kl ? adc::kPgKlPieces : 0)) * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (kl) kl_stats_minibatch(e, 0, sums + adc::kPgSums, S);
    const adc::PgStatsOut st = adc::pg_stats_finish(sums, S);
    if (g && !sh_minibatch_evaluated(e, 0, st.approx_kl, S)) {     // (stops here: no step, the count stays)
        if (out) *out = st;
        return ADC_OK;
    }
    const bool clip = e->pg_cfg.max_grad_norm > 0.0f;
    const float scale = clip ? adc::pg_clip_scale(e->pg_cfg.max_grad_norm, st.grad_norm) : 1.0f;
    hipLaunchKernelGGL(k_pg_update, dim3((unsigned)((Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->pg_lay, e->pg_theta, e->pg_m,
                       e->pg_v, e->pg_grad, clip ? 1 : 0, scale, pg_step_of(e->pg_cfg, e->pg_steps));
    HIP_TRY(hipGetLastError());
    e->pg_steps += 1;
    if (out) *out = st;
    return ADC_OK;
}

void pg_stats_fill(adc_pg_stats *stats, const adc::PgStatsOut &o, int64_t steps, int64_t samples)
{
    stats->steps = steps; stats->samples = samples;
    stats->policy_loss = o.policy_loss; stats->value_loss = o.value_loss; stats->entropy = o.entropy; stats->approx_kl = o.approx_kl;
    stats->clip_fraction = o.clip_fraction; stats->grad_norm = o.grad_norm; stats->explained_variance = o.explained_variance;
}
}  // namespace

ADC_EXPORT int adc_engine_pg_init(adc_engine *e, const adc_pg_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_pg_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = pg_state_check(e)) return rc;
    if (e->have_td3 || e->have_td3_pop) return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_sac || e->have_sac_pop) return fail(ADC_ESTATE, "a soft actor-critic trainer is alive on this engine: one trainer at a time owns the policy's weights");
    const int N = e->v.N, mb = cfg->minibatch_envs == 0 ? N : cfg->minibatch_envs;
    if (mb > N || N % mb != 0) return fail(ADC_EINVAL, "minibatch_envs must divide num_envs");
    if (pg_chunks((long long)e->ro_T * mb) > 65535) return fail(ADC_EINVAL, "horizon x minibatch_envs: at most 65535 x 1024 samples in a minibatch");
    const adc::PgShape sh = adc::pg_shape_of(e->mlp_cfg, e->v.K, mlp_frames(e));
    int maxw = 1;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) maxw = std::max(maxw, sh.n_out[net][l]);
    if (pg_lds_floats(sh, maxw) * sizeof(float) > 64u * 1024u)
        return fail(ADC_EINVAL, pg_lds_floats(adc::pg_shape_of(e->mlp_cfg, e->v.K), maxw) * sizeof(float) > 64u * 1024u
                                    ? "num_keywords too large for policy-gradient training (LDS)"
                                    : "frames: the stacked input row is too large for policy-gradient training (LDS); fewer frames fit");
    ENGINE_GUARD(e);
    // the flat order against the device's stores
    PgLayout lay{};
    {
        int flat = 0, i = 0;
        for (int net = 0; net < 2; ++net) {
            const MlpNet &n = net == 0 ? e->mp.pol : e->mp.val;
            for (int l = 0; l < sh.layers[net]; ++l, ++i) {
                lay.flat0[i] = flat; lay.n_in[i] = n.n_in[l]; lay.n_out[i] = n.n_out[l];
                lay.W[i] = const_cast<float *>(n.W[l]); lay.b[i] = const_cast<float *>(n.b[l]);
                flat += (n.n_in[l] + 1) * n.n_out[l];
            }
        }
        if (!sh.two_heads) {
            lay.flat0[i] = flat; lay.n_in[i] = 0; lay.n_out[i] = sh.A; lay.W[i] = nullptr; lay.b[i] = const_cast<float *>(e->mp.log_std);
            flat += sh.A; ++i;
        }
        lay.nterms = i; lay.Q = flat;
    }
    const size_t Q = (size_t)lay.Q, tn = (size_t)e->ro_T * (size_t)N, smax = (size_t)e->ro_T * (size_t)mb;
    const size_t parts = (size_t)pg_chunks((long long)std::max(tn, Q)) * 8u + 8u;
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *adv = nullptr, *ret = nullptr, *acts = nullptr, *deltas = nullptr, *pieces = nullptr;
    double *part = nullptr, *sums = nullptr, *gpart = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &theta, Q)) || (rc = mlp_alloc(e, fresh, &m, Q)) || (rc = mlp_alloc(e, fresh, &v, Q)) ||
        (rc = mlp_alloc(e, fresh, &grad, Q)) || (rc = mlp_alloc(e, fresh, &adv, tn)) || (rc = mlp_alloc(e, fresh, &ret, tn)) ||
        (rc = mlp_alloc(e, fresh, &acts, smax * (size_t)adc::pg_acts_floats(sh))) || (rc = mlp_alloc(e, fresh, &deltas, smax * (size_t)adc::pg_deltas_floats(sh))) ||
        (rc = mlp_alloc(e, fresh, &pieces, smax * (size_t)adc::kPgPieces)) || (rc = mlp_alloc(e, fresh, &part, parts)) ||
        (rc = mlp_alloc(e, fresh, &gpart, (size_t)pg_chunks((long long)smax) * Q)) ||
        (rc = mlp_alloc(e, fresh, &sums, (size_t)16))) {
        // (rc and its message are mlp_alloc's: ADC_ENOMEM for a refused allocation, ADC_EHIP for a failed memset; no test provokes either)
        mlp_free(e, fresh);
        return rc;
    }
    pg_drop(e);
    e->pg_allocs.swap(fresh);
    e->pg_theta = theta; e->pg_m = m; e->pg_v = v; e->pg_grad = grad; e->pg_adv = adv; e->pg_ret = ret;
    e->pg_acts = acts; e->pg_deltas = deltas; e->pg_pieces = pieces; e->pg_part = part; e->pg_sums = sums; e->pg_gpart = gpart;
    e->pg_cfg = *cfg; e->pg_mb = mb; e->pg_slots = smax; e->pg_shape = sh; e->pg_lay = lay; e->pg_maxw = maxw;
    // theta starts as the device's weights
    hipLaunchKernelGGL(k_pg_params_copy, dim3((unsigned)((lay.Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, lay, e->pg_theta, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_pg = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_param_count(adc_engine *e, int64_t *count)
{
    if (!e || !count) return fail(ADC_EINVAL, "engine handle or count is NULL");
    if (int rc = pg_ready(e)) return rc;
    *count = e->pg_lay.Q;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_advantages(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e)) || (rc = pg_state_check(e)) || (rc = pg_record_check(e))) return rc;
    ENGINE_GUARD(e);
    return pg_advantages_run(e);
}

ADC_EXPORT int adc_engine_pg_advantages_fetch(adc_engine *e, float *adv_tn, float *ret_tn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pg_ready(e)) return rc;
    if (!e->pg_adv_ready) return fail(ADC_ESTATE, "adc_engine_pg_advantages has not been called since the last recorded day");
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->ro_t * (size_t)e->v.N * 4;
    if (adv_tn) HIP_TRY(hipMemcpyAsync(adv_tn, e->pg_adv, bytes, hipMemcpyDeviceToHost, e->stream));
    if (ret_tn) HIP_TRY(hipMemcpyAsync(ret_tn, e->pg_ret, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_minibatch(adc_engine *e, int32_t env_begin, int32_t env_count, adc_pg_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e)) || (rc = pg_state_check(e)) || (rc = pg_record_check(e))) return rc;
    if (!e->pg_adv_ready) return fail(ADC_ESTATE, "adc_engine_pg_advantages has not been called since the last recorded day");
    if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > e->v.N) return fail(ADC_EINVAL, "the env range is not inside [0, num_envs)");
    if (env_count > e->pg_mb) return fail(ADC_EINVAL, "env_count exceeds the configuration's minibatch_envs (the scratch was sized for it)");
    ENGINE_GUARD(e);
    adc::PgStatsOut o;
    if ((rc = pg_minibatch_run(e, env_begin, env_count, &o, nullptr))) return rc;
    if (stats) pg_stats_fill(stats, o, e->pg_steps, (int64_t)e->ro_t * env_count);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_update(adc_engine *e, int32_t epochs, adc_pg_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e)) || (rc = pg_state_check(e)) || (rc = pg_record_check(e))) return rc;
    if (epochs < 1 || epochs > 65536) return fail(ADC_EINVAL, "epochs: 1 to 65536");
    ENGINE_GUARD(e);
    if ((rc = pg_advantages_run(e))) return rc;
    if (e->sh_live) return sh_update_run(e, epochs, stats);
    const int N = e->v.N, mb = e->pg_mb, count = N / mb;
    adc::PgStatsOut mean{};
    KlEpoch kl;
    for (int ep = 0; ep < epochs; ++ep) {
        adc::PgStatsOut acc{};
        kl.begin(e);
        for (int i = 0; i < count; ++i) {
            adc::PgStatsOut o;
            if ((rc = pg_minibatch_run(e, i * mb, mb, &o, nullptr))) return rc;
            kl.add(e);
            acc.policy_loss = acc.policy_loss + o.policy_loss; acc.value_loss = acc.value_loss + o.value_loss; acc.entropy = acc.entropy + o.entropy;
            acc.approx_kl = acc.approx_kl + o.approx_kl; acc.clip_fraction = acc.clip_fraction + o.clip_fraction;
            acc.grad_norm = acc.grad_norm + o.grad_norm; acc.explained_variance = acc.explained_variance + o.explained_variance;
        }
        const double c = (double)count;
        mean = adc::PgStatsOut{acc.policy_loss / c, acc.value_loss / c, acc.entropy / c, acc.approx_kl / c, acc.clip_fraction / c, acc.grad_norm / c,
                               acc.explained_variance / c};
    }
    if (e->kl_live && (rc = kl_update_end(e, kl))) return rc;
    if (stats) pg_stats_fill(stats, mean, e->pg_steps, (int64_t)e->ro_t * mb);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_state_get(adc_engine *e, float *theta_q, float *m_q, float *v_q, int64_t *steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pg_ready(e)) return rc;
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->pg_lay.Q * 4;
    if (theta_q) HIP_TRY(hipMemcpyAsync(theta_q, e->pg_theta, bytes, hipMemcpyDeviceToHost, e->stream));
    if (m_q) HIP_TRY(hipMemcpyAsync(m_q, e->pg_m, bytes, hipMemcpyDeviceToHost, e->stream));
    if (v_q) HIP_TRY(hipMemcpyAsync(v_q, e->pg_v, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (steps) *steps = e->pg_steps;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_state_set(adc_engine *e, const float *theta_q, const float *m_q, const float *v_q, int64_t steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pg_ready(e)) return rc;
    if (!theta_q || !m_q || !v_q) return fail(ADC_EINVAL, "theta, m or v is NULL");
    if (steps < 0 || steps >= 0x7FFFFFFFll) return fail(ADC_EINVAL, "steps: 0 to 2^31 - 2");
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->pg_lay.Q * 4;
    HIP_TRY(hipMemcpyAsync(e->pg_theta, theta_q, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_m, m_q, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_v, v_q, bytes, hipMemcpyHostToDevice, e->stream));
    // (the device's layers and log_std follow theta, so that the next act and the next recorded day see it)
    hipLaunchKernelGGL(k_pg_params_copy, dim3((unsigned)((e->pg_lay.Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->pg_lay, e->pg_theta, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pg_steps = steps;
    return ADC_OK;
}

// ---- learner populations: M PPO / A2C learners in lock-step, every launch over all members (include/adcraft_engine.h) ----------
namespace {
int pgp_ready(const adc_engine *e)
{
    if (!e->have_pg_pop)
        return fail(ADC_ESTATE, "adc_engine_pg_pop_init has not been called (or the policy, the learners or the record were re-initialised since)");
    return ADC_OK;
}
int pgp_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (e->lrn_M == 0) return fail(ADC_ESTATE, "population training needs learners (adc_engine_mlp_learners)");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "policy-gradient training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "policy-gradient training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
int pgp_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= e->lrn_M) return fail(ADC_EINVAL, "no such member");
    return ADC_OK;
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

int pgp_advantages_run(adc_engine *e)
{
    const int N = e->v.N, T = e->ro_t, M = e->lrn_M, n = e->lrn_n;
    const long long tn = (long long)T * N;
    int rc;
    if (e->mp.val.layers > 0)
        mlp_launch_kernel(e->v, e->mp, e->stream, 1, nullptr, 0.0f, e->d_bids, e->d_budget, MlpRecordSlot{nullptr, nullptr, nullptr, nullptr}, e->mlp_boot);
    else HIP_TRY(hipMemsetAsync(e->mlp_boot, 0, (size_t)N * 4, e->stream));
    if (e->rn.live)       // (the reward times the env's normaliser's multiplier, clipped: adc_rew_norm.h)
        hipLaunchKernelGGL(k_rew_norm_pop_gae, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, N, T, n, e->pgp_dmem, e->ro_reward, e->ro_term,
                           e->ro_trunc, e->ro_value, e->mlp_boot, e->rn.rew.scale, N / e->rn.M, e->rn_cfg.clip, e->pg_adv, e->pg_ret);
    else
        hipLaunchKernelGGL(k_pg_pop_gae, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, N, T, n, e->pgp_dmem, e->ro_reward, e->ro_term, e->ro_trunc,
                           e->ro_value, e->mlp_boot, e->pg_adv, e->pg_ret);
    HIP_TRY(hipGetLastError());
    bool any = false;
    for (const PgMember &m : e->pgp_mem) any = any || m.normalize;
    if (any) {
        // the law's two passes per member over its T n samples in its own order i = t * n + local env; the moments finished on
        // the host as the solo path's are, all members' in one copy each way
        const int cnt = T * n;
        if ((rc = pgp_csum_launch(e, e->pg_adv, cnt, n, N, (size_t)n, 1, 1, 0, 0)) || (rc = pgp_sums_fetch(e))) return rc;
        for (int m = 0; m < M; ++m) e->pgp_mem[(size_t)m].mean = e->pgp_host_sums[(size_t)m * 16] / (double)cnt;
        if ((rc = pgp_members_upload(e)) || (rc = pgp_csum_launch(e, e->pg_adv, cnt, n, N, (size_t)n, 1, 1, 1, 0)) || (rc = pgp_sums_fetch(e))) return rc;
        for (int m = 0; m < M; ++m) e->pgp_mem[(size_t)m].sd = std::sqrt(e->pgp_host_sums[(size_t)m * 16] / (double)cnt);
        if ((rc = pgp_members_upload(e))) return rc;
        hipLaunchKernelGGL(k_pg_pop_normalize, dim3((unsigned)((tn + 255) / 256)), dim3(256), 0, e->stream, e->pg_adv, tn, N, n, e->pgp_dmem);
        HIP_TRY(hipGetLastError());
    }
    if (e->kl_live)
        if ((rc = kl_snapshot_launch(e))) return rc;
    if (e->sh_live) sh_update_begin(e);
    e->pg_adv_ready = true;
    return ADC_OK;
}

// minibatch `index` of every member: one gradient and one step each, in the same launches - or, g given (shuffled minibatches), over
// the g->S samples of every member whose record rows are g->rows + member * g->stride; a member whose update has stopped is covered
// by the launches and left as it is
int pgp_minibatch_run(adc_engine *e, int index, adc::PgStatsOut *out_m, const PgGather *g)
{
    const adc::PgShape &sh = e->pg_shape;
    const int N = e->v.N, T = e->ro_t, M = e->lrn_M, n = e->lrn_n, B = e->pg_mb, n0 = index * B;
    const int na = adc::pg_acts_floats(sh), nd = adc::pg_deltas_floats(sh), Q = e->lrn_lay.Q;
    const long long S = g ? g->S : (long long)T * B;
    const unsigned chunks = (unsigned)pg_chunks(S);
    PgView p{};
    p.sh = sh;
    p.obs = e->ro_obs; p.action = e->ro_action; p.logp = e->ro_logp; p.value = e->ro_value;
    p.adv = e->pg_adv; p.ret = e->pg_ret;
    p.N = N; p.n0 = n0; p.B = B;
    p.acts = e->pg_acts; p.deltas = e->pg_deltas; p.pieces = e->pg_pieces;
    p.na = na; p.nd = nd; p.maxw = e->pg_maxw;
    const bool kl = e->kl_live;
    if (g && kl)
        hipLaunchKernelGGL(k_pg_pop_gather_kl_sample, dim3((unsigned)S, (unsigned)M), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw, true) * sizeof(float),
                           e->stream, p, kl_view(e), e->lrn_tab, e->pgp_dmem, e->kl_dmem, g->rows, g->stride);
    else if (g)
        hipLaunchKernelGGL(k_pg_pop_gather_sample, dim3((unsigned)S, (unsigned)M), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw) * sizeof(float), e->stream, p,
                           e->lrn_tab, e->pgp_dmem, g->rows, g->stride);
    else if (kl)
        hipLaunchKernelGGL(k_pg_pop_kl_sample, dim3((unsigned)S, (unsigned)M), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw, true) * sizeof(float), e->stream, p,
                           kl_view(e), e->lrn_tab, e->pgp_dmem, e->kl_dmem, n);
    else
        hipLaunchKernelGGL(k_pg_pop_sample, dim3((unsigned)S, (unsigned)M), dim3(kPgBlock), pg_lds_floats(sh, e->pg_maxw) * sizeof(float), e->stream, p,
                           e->lrn_tab, e->pgp_dmem, n);
    {
        int flat = 0, ao = 0, dof = 0;
        auto launch = [&](const float *X, size_t ldx, int n_in, int n_out, int obs) {
            PgTerm t{X, ldx, n_in, n_out, dof, flat, obs};
            const unsigned tiles = (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile));
            if (g)
                hipLaunchKernelGGL(k_pg_pop_gather_wgrad, dim3(tiles, chunks, (unsigned)M), dim3(kPgBlock), 0, e->stream, t, S, g->rows, g->stride, e->pg_deltas,
                                   nd, e->pg_gpart, Q);
            else
                hipLaunchKernelGGL(k_pg_pop_wgrad, dim3(tiles, chunks, (unsigned)M), dim3(kPgBlock), 0, e->stream, t, S, B, N, n0, n, e->pg_deltas, nd, e->pg_gpart, Q);
            flat += (n_in + 1) * n_out;
        };
        for (int net = 0; net < 2; ++net)
            for (int l = 0; l < sh.layers[net]; ++l) {
                const int n_in = adc::pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
                if (l == 0) launch(e->ro_obs, (size_t)sh.D, n_in, n_out, 1);
                else { launch(e->pg_acts + ao, (size_t)na, n_in, n_out, 0); ao += n_in; }
                dof += n_out;
            }
        if (!sh.two_heads) launch(nullptr, 0, 0, sh.A, 0);
    }
    hipLaunchKernelGGL(k_pg_pop_grad_join, dim3(pg_blocks(Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, e->pg_gpart, (int)chunks, Q, S, e->pg_grad);
    HIP_TRY(hipGetLastError());
    int rc;
    if ((rc = pgp_csum_launch(e, e->pg_pieces, (int)S, 0, 0, (size_t)S, adc::kPgPieces, 7, 0, 0)) ||
        (rc = pgp_csum_launch(e, e->pg_pieces + adc::kPgRet, (int)S, 0, 0, (size_t)S, adc::kPgPieces, 2, 2, 7)) ||
        (rc = pgp_csum_launch(e, e->pg_grad, Q, 0, 0, (size_t)Q, 1, 1, 2, 9)) ||
        (kl && (rc = pgp_csum_launch(e, e->kl_pieces, (int)S, 0, 0, (size_t)S, adc::kPgKlPieces, adc::kPgKlPieces, 0, adc::kPgSums))) || (rc = pgp_sums_fetch(e)))
        return rc;
    // the statistics, the clip scale and the step's constants of every member on the host, as the solo path's are; up in one copy
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
    if (g) {
        hipLaunchKernelGGL(k_pg_pop_update_live, dim3(pg_blocks(Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, e->pg_theta, e->pg_m,
                           e->pg_v, e->pg_grad, e->pgp_dmem);
        HIP_TRY(hipGetLastError());
        for (int m = 0; m < M; ++m)
            if (!e->pgp_mem[(size_t)m].stopped) e->pgp_steps[(size_t)m] += 1;
        return ADC_OK;
    }
    hipLaunchKernelGGL(k_pg_pop_update, dim3(pg_blocks(Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, e->pg_theta, e->pg_m, e->pg_v,
                       e->pg_grad, e->pgp_dmem);
    HIP_TRY(hipGetLastError());
    // (no wait here, as in the solo path: whoever writes the host's table next has waited for the stream since this upload - the
    //  sums' fetch of the next minibatch or normalisation pass, or adc_engine_pg_pop_set_config's own wait)
    for (int m = 0; m < M; ++m) e->pgp_steps[(size_t)m] += 1;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_pg_pop_init(adc_engine *e, const adc_pg_config *cfgs, int32_t count)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pgp_state_check(e)) return rc;
    const int N = e->v.N, M = e->lrn_M, n = e->lrn_n;
    const char *why = nullptr;
    if (adc_pg_pop_config_check(cfgs, count, N, M, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (e->have_td3 || e->have_td3_pop) return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_sac || e->have_sac_pop) return fail(ADC_ESTATE, "a soft actor-critic trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_pg) return fail(ADC_ESTATE, "a single-learner trainer is alive on this engine (adc_engine_pg_init)");
    const int mb = cfgs[0].minibatch_envs == 0 ? n : cfgs[0].minibatch_envs;
    if (pg_chunks((long long)e->ro_T * n) > 65535) return fail(ADC_EINVAL, "horizon x envs of a member: at most 65535 x 1024 samples");
    if (pg_chunks((long long)e->ro_T * mb) > 65535) return fail(ADC_EINVAL, "horizon x minibatch_envs: at most 65535 x 1024 samples in a minibatch");
    // (the member is the grid's y or z: adc_engine_mlp_learners admits at most 65535)
    const adc::PgShape sh = adc::pg_shape_of(e->mlp_cfg, e->v.K, mlp_frames(e));
    int maxw = 1;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) maxw = std::max(maxw, sh.n_out[net][l]);
    if (pg_lds_floats(sh, maxw) * sizeof(float) > 64u * 1024u)
        return fail(ADC_EINVAL, pg_lds_floats(adc::pg_shape_of(e->mlp_cfg, e->v.K), maxw) * sizeof(float) > 64u * 1024u
                                    ? "num_keywords too large for policy-gradient training (LDS)"
                                    : "frames: the stacked input row is too large for policy-gradient training (LDS); fewer frames fit");
    ENGINE_GUARD(e);
    const size_t Q = (size_t)e->lrn_lay.Q, tn = (size_t)e->ro_T * (size_t)N, smax = (size_t)e->ro_T * (size_t)mb, Ms = (size_t)M;
    const size_t part_stride = (size_t)pg_chunks((long long)std::max((size_t)e->ro_T * (size_t)n, Q)) * 8u + 8u;
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *adv = nullptr, *ret = nullptr, *acts = nullptr, *deltas = nullptr, *pieces = nullptr;
    double *part = nullptr, *sums = nullptr, *gpart = nullptr;
    PgMember *dmem = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &theta, Ms * Q)) || (rc = mlp_alloc(e, fresh, &m, Ms * Q)) || (rc = mlp_alloc(e, fresh, &v, Ms * Q)) ||
        (rc = mlp_alloc(e, fresh, &grad, Ms * Q)) || (rc = mlp_alloc(e, fresh, &adv, tn)) || (rc = mlp_alloc(e, fresh, &ret, tn)) ||
        (rc = mlp_alloc(e, fresh, &acts, Ms * smax * (size_t)adc::pg_acts_floats(sh))) ||
        (rc = mlp_alloc(e, fresh, &deltas, Ms * smax * (size_t)adc::pg_deltas_floats(sh))) ||
        (rc = mlp_alloc(e, fresh, &pieces, Ms * smax * (size_t)adc::kPgPieces)) || (rc = mlp_alloc(e, fresh, &part, Ms * part_stride)) ||
        (rc = mlp_alloc(e, fresh, &gpart, Ms * (size_t)pg_chunks((long long)smax) * Q)) || (rc = mlp_alloc(e, fresh, &sums, Ms * 16u)) ||
        (rc = mlp_alloc(e, fresh, &dmem, Ms))) {
        mlp_free(e, fresh);
        return rc;
    }
    pg_drop(e);
    e->pg_allocs.swap(fresh);
    e->pg_theta = theta; e->pg_m = m; e->pg_v = v; e->pg_grad = grad; e->pg_adv = adv; e->pg_ret = ret;
    e->pg_acts = acts; e->pg_deltas = deltas; e->pg_pieces = pieces; e->pg_part = part; e->pg_sums = sums; e->pg_gpart = gpart;
    e->pg_mb = mb; e->pg_slots = smax; e->pg_shape = sh; e->pg_maxw = maxw;
    e->pgp_dmem = dmem; e->pgp_part_stride = part_stride;
    e->pgp_cfg.assign(Ms, cfgs[0]);
    if (count > 1) e->pgp_cfg.assign(cfgs, cfgs + M);
    e->pgp_steps.assign(Ms, 0);
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

ADC_EXPORT int adc_engine_pg_pop_advantages(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_state_check(e)) || (rc = pg_record_check(e))) return rc;
    ENGINE_GUARD(e);
    return pgp_advantages_run(e);
}

ADC_EXPORT int adc_engine_pg_pop_advantages_fetch(adc_engine *e, float *adv_tn, float *ret_tn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pgp_ready(e)) return rc;
    if (!e->pg_adv_ready) return fail(ADC_ESTATE, "adc_engine_pg_pop_advantages has not been called since the last recorded day");
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->ro_t * (size_t)e->v.N * 4;
    if (adv_tn) HIP_TRY(hipMemcpyAsync(adv_tn, e->pg_adv, bytes, hipMemcpyDeviceToHost, e->stream));
    if (ret_tn) HIP_TRY(hipMemcpyAsync(ret_tn, e->pg_ret, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_minibatch(adc_engine *e, int32_t index, adc_pg_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_state_check(e)) || (rc = pg_record_check(e))) return rc;
    if (!e->pg_adv_ready) return fail(ADC_ESTATE, "adc_engine_pg_pop_advantages has not been called since the last recorded day");
    if (index < 0 || index >= e->lrn_n / e->pg_mb) return fail(ADC_EINVAL, "no such minibatch: 0 to envs of a member / minibatch_envs - 1");
    ENGINE_GUARD(e);
    std::vector<adc::PgStatsOut> o((size_t)e->lrn_M);
    if ((rc = pgp_minibatch_run(e, index, o.data(), nullptr))) return rc;
    if (stats_m)
        for (int m = 0; m < e->lrn_M; ++m) pg_stats_fill(stats_m + m, o[(size_t)m], e->pgp_steps[(size_t)m], (int64_t)e->ro_t * e->pg_mb);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_update(adc_engine *e, int32_t epochs, adc_pg_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_state_check(e)) || (rc = pg_record_check(e))) return rc;
    if (epochs < 1 || epochs > 65536) return fail(ADC_EINVAL, "epochs: 1 to 65536");
    ENGINE_GUARD(e);
    if ((rc = pgp_advantages_run(e))) return rc;
    if (e->sh_live) return sh_update_run(e, epochs, stats_m);
    const int M = e->lrn_M, count = e->lrn_n / e->pg_mb;
    std::vector<adc::PgStatsOut> o((size_t)M), acc((size_t)M), mean((size_t)M);
    KlEpoch kl;
    for (int ep = 0; ep < epochs; ++ep) {
        acc.assign((size_t)M, adc::PgStatsOut{});
        kl.begin(e);
        for (int i = 0; i < count; ++i) {
            if ((rc = pgp_minibatch_run(e, i, o.data(), nullptr))) return rc;
            kl.add(e);
            for (size_t m = 0; m < (size_t)M; ++m) {
                adc::PgStatsOut &a = acc[m];
                a.policy_loss = a.policy_loss + o[m].policy_loss; a.value_loss = a.value_loss + o[m].value_loss; a.entropy = a.entropy + o[m].entropy;
                a.approx_kl = a.approx_kl + o[m].approx_kl; a.clip_fraction = a.clip_fraction + o[m].clip_fraction;
                a.grad_norm = a.grad_norm + o[m].grad_norm; a.explained_variance = a.explained_variance + o[m].explained_variance;
            }
        }
        const double c = (double)count;
        for (size_t m = 0; m < (size_t)M; ++m) {
            const adc::PgStatsOut &a = acc[m];
            mean[m] = adc::PgStatsOut{a.policy_loss / c, a.value_loss / c, a.entropy / c, a.approx_kl / c, a.clip_fraction / c, a.grad_norm / c,
                                      a.explained_variance / c};
        }
    }
    if (e->kl_live && (rc = kl_update_end(e, kl))) return rc;       // (every member's adaptation: one small upload)
    if (stats_m)
        for (int m = 0; m < M; ++m) pg_stats_fill(stats_m + m, mean[(size_t)m], e->pgp_steps[(size_t)m], (int64_t)e->ro_t * e->pg_mb);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_state_get(adc_engine *e, int32_t member, float *theta_q, float *m_q, float *v_q, int64_t *steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    const size_t Q = (size_t)e->lrn_lay.Q, bytes = Q * 4, at = (size_t)member * Q;
    if (theta_q) HIP_TRY(hipMemcpyAsync(theta_q, e->pg_theta + at, bytes, hipMemcpyDeviceToHost, e->stream));
    if (m_q) HIP_TRY(hipMemcpyAsync(m_q, e->pg_m + at, bytes, hipMemcpyDeviceToHost, e->stream));
    if (v_q) HIP_TRY(hipMemcpyAsync(v_q, e->pg_v + at, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (steps) *steps = e->pgp_steps[(size_t)member];
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_state_set(adc_engine *e, int32_t member, const float *theta_q, const float *m_q, const float *v_q, int64_t steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_member_check(e, member))) return rc;
    if (!theta_q || !m_q || !v_q) return fail(ADC_EINVAL, "theta, m or v is NULL");
    if (steps < 0 || steps >= 0x7FFFFFFFll) return fail(ADC_EINVAL, "steps: 0 to 2^31 - 2");
    ENGINE_GUARD(e);
    const size_t Q = (size_t)e->lrn_lay.Q, bytes = Q * 4, at = (size_t)member * Q;
    HIP_TRY(hipMemcpyAsync(e->pg_theta + at, theta_q, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_m + at, m_q, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_v + at, v_q, bytes, hipMemcpyHostToDevice, e->stream));
    // (the member's layers and log_std follow its theta, so that the next act and the next recorded day see it)
    hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks((int)Q), 1u), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, (int)member,
                       e->pg_theta + at, (size_t)0, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pgp_steps[(size_t)member] = steps;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_pop_set_config(adc_engine *e, int32_t member, const adc_pg_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_member_check(e, member))) return rc;
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
    if ((rc = pgp_ready(e)) || (rc = pgp_member_check(e, src)) || (rc = pgp_member_check(e, dst))) return rc;
    if (src == dst) return ADC_OK;
    ENGINE_GUARD(e);
    const size_t Q = (size_t)e->lrn_lay.Q, bytes = Q * 4, from = (size_t)src * Q, to = (size_t)dst * Q;
    HIP_TRY(hipMemcpyAsync(e->pg_theta + to, e->pg_theta + from, bytes, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_m + to, e->pg_m + from, bytes, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_v + to, e->pg_v + from, bytes, hipMemcpyDeviceToDevice, e->stream));
    hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks((int)Q), 1u), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, (int)dst, e->pg_theta + to,
                       (size_t)0, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pgp_steps[(size_t)dst] = e->pgp_steps[(size_t)src];
    if ((rc = kl_copy(e, 1, [&](int, int &d, int &f) { d = dst; f = src; }))) return rc;      // (the donor's KL coefficient)
    return ADC_OK;
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

// pg_minibatch_run / pgp_minibatch_run without the host in the middle: minibatch `index` of an epoch (g given: the gathered one) of
// every member, its decision and its step enqueued; row `serial` of the log takes its sums
int pq_minibatch_enqueue(adc_engine *e, const PqPlan &pl, int index, int serial, const PgGather *g)
{
    const adc::PgShape &sh = e->pg_shape;
    const bool pop = e->have_pg_pop, kl = e->kl_live;
    const int N = e->v.N, T = e->ro_t, M = pl.M, n = sh_member_envs(e), B = g ? 1 : e->pg_mb, n0 = g ? 0 : index * B;
    const int na = adc::pg_acts_floats(sh), nd = adc::pg_deltas_floats(sh), Q = pop ? e->lrn_lay.Q : e->pg_lay.Q;
    const long long S = g ? g->S : (long long)T * B;
    const unsigned chunks = (unsigned)pg_chunks(S);
    const PgQCtl *ctl = reinterpret_cast<const PgQCtl *>(e->pq_dev + pl.ctl);
    PgView p{};
    p.sh = sh;
    if (!pop) {
        p.loss = adc::PgLoss{e->pg_cfg.eps_clip, e->pg_cfg.vf_coef, e->pg_cfg.ent_coef};
        p.net[0] = e->mp.pol; p.net[1] = e->mp.val;
        p.log_std = e->mp.log_std;
    }
    p.obs = e->ro_obs; p.action = e->ro_action; p.logp = e->ro_logp; p.value = e->ro_value;
    p.adv = e->pg_adv; p.ret = e->pg_ret;
    p.N = N; p.n0 = n0; p.B = B;
    p.acts = e->pg_acts; p.deltas = e->pg_deltas; p.pieces = e->pg_pieces;
    p.na = na; p.nd = nd; p.maxw = e->pg_maxw;
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
    // the gradient's terms in the flat order
    {
        int flat = 0, ao = 0, dof = 0;
        auto launch = [&](const float *X, size_t ldx, int n_in, int n_out, int obs) {
            PgTerm t{X, ldx, n_in, n_out, dof, flat, obs};
            const unsigned tiles = (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile));
            if (pop && g)
                hipLaunchKernelGGL(k_pg_pop_q_gather_wgrad, dim3(tiles, chunks, (unsigned)M), blk, 0, e->stream, t, S, g->rows, g->stride, e->pg_deltas, nd,
                                   e->pg_gpart, Q, ctl);
            else if (pop)
                hipLaunchKernelGGL(k_pg_pop_q_wgrad, dim3(tiles, chunks, (unsigned)M), blk, 0, e->stream, t, S, B, N, n0, n, e->pg_deltas, nd, e->pg_gpart, Q, ctl);
            else if (g)
                hipLaunchKernelGGL(k_pg_q_gather_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, g->rows, e->pg_deltas, nd, e->pg_gpart, Q, ctl);
            else
                hipLaunchKernelGGL(k_pg_q_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, B, N, n0, e->pg_deltas, nd, e->pg_gpart, Q, ctl);
            flat += (n_in + 1) * n_out;
        };
        for (int net = 0; net < 2; ++net)
            for (int l = 0; l < sh.layers[net]; ++l) {
                const int n_in = adc::pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
                if (l == 0) launch(e->ro_obs, (size_t)sh.D, n_in, n_out, 1);
                else { launch(e->pg_acts + ao, (size_t)na, n_in, n_out, 0); ao += n_in; }
                dof += n_out;
            }
        if (!sh.two_heads) launch(nullptr, 0, 0, sh.A, 0);
    }
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
    const int M = sh_members(e), n = sh_member_envs(e), N = e->v.N;
    const uint32_t n_s = (uint32_t)e->ro_t * (uint32_t)n;
    if (shuffle) e->sh_ns = n_s;
    const int count = shuffle ? sh_minibatches(e) : n / e->pg_mb;
    if ((long long)epochs * count > (1ll << 22)) return fail(ADC_EINVAL, "epochs x minibatches: at most 2^22 steps in one queued update (its log and step tables)");
    const PqPlan pl = pq_plan(M, epochs, count, shuffle);
    int rc;
    if ((rc = pq_reserve(e, pl.end))) return rc;
    auto steps0 = [&](int m) { return pop ? e->pgp_steps[(size_t)m] : e->pg_steps; };
    // 2. the tables, up once
    std::memset(e->pq_host, 0, pl.log);
    PgQLaw *law = reinterpret_cast<PgQLaw *>(e->pq_host + pl.law);
    adc::EsStep *steps = reinterpret_cast<adc::EsStep *>(e->pq_host + pl.steps);
    PgShuffleMember *ticks = reinterpret_cast<PgShuffleMember *>(e->pq_host + pl.ticks);
    for (int m = 0; m < M; ++m) {
        const adc_pg_config &c = pop ? e->pgp_cfg[(size_t)m] : e->pg_cfg;
        law[m] = PgQLaw{c.max_grad_norm, shuffle ? e->sh_cfg[(size_t)m].target_kl : 0.0f};
        pq_steps_fill(steps + (size_t)m * (size_t)pl.cap, c, steps0(m), pl.cap);
        if (shuffle)
            for (int ep = 0; ep < epochs; ++ep) {       // (a live member has taken exactly ep * count steps of this update when epoch ep begins)
                PgShuffleMember &t = ticks[(size_t)ep * (size_t)M + (size_t)m];
                t.key = e->sh_mem[(size_t)m].key;
                t.tick = (uint32_t)((uint64_t)(steps0(m) + (int64_t)ep * count) & 0xFFFFFFFFull);
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
                    sh_stats_add(acc[(size_t)m], adc::pg_stats_finish(r.sums, r.count));
                    taken[(size_t)m] += 1;
                }
                klep.add(e);
            }
            for (int m = 0; m < M; ++m) mean[(size_t)m] = sh_stats_mean(acc[(size_t)m], count);
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
                    sh_stats_add(acc[(size_t)m], st);
                    cnt[(size_t)m] += 1;
                }
                klep.add(e, e->sh_evaluated.data());
            }
            for (int m = 0; m < M; ++m)
                if (live[(size_t)m]) mean[(size_t)m] = sh_stats_mean(acc[(size_t)m], cnt[(size_t)m]);
        }
        e->sh_epoch_ready = false;      // (the chain drew every epoch's order over the last one's: none of them is kept for a later call)
    }
    for (int m = 0; m < M; ++m) {
        agree = agree && ctl[m].taken == taken[(size_t)m] && (ctl[m].stopped != 0) == (shuffle && e->sh_stats[(size_t)m].stopped);
        if (pop) e->pgp_steps[(size_t)m] += taken[(size_t)m];
        else e->pg_steps += taken[(size_t)m];
    }
    // (one law, two sides: a difference would mean the device took steps the host's statistics do not describe - never silently)
    if (!agree) return fail(ADC_EHIP, "the queued update's device decisions and their replay on the host disagree");
    if (kl && (rc = kl_update_end(e, klep, true))) return rc;
    if (stats_m)
        for (int m = 0; m < M; ++m)
            pg_stats_fill(stats_m + m, mean[(size_t)m], steps0(m), shuffle ? e->sh_last_count[(size_t)m] : (int64_t)e->ro_t * e->pg_mb);
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_pg_update_queued(adc_engine *e, int32_t epochs, adc_pg_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e)) || (rc = pg_state_check(e)) || (rc = pg_record_check(e))) return rc;
    if (epochs < 1 || epochs > 65536) return fail(ADC_EINVAL, "epochs: 1 to 65536");
    ENGINE_GUARD(e);
    if ((rc = pg_advantages_run(e))) return rc;
    return pq_update_run(e, epochs, stats);
}

ADC_EXPORT int adc_engine_pg_pop_update_queued(adc_engine *e, int32_t epochs, adc_pg_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pgp_ready(e)) || (rc = pgp_state_check(e)) || (rc = pg_record_check(e))) return rc;
    if (epochs < 1 || epochs > 65536) return fail(ADC_EINVAL, "epochs: 1 to 65536");
    ENGINE_GUARD(e);
    if ((rc = pgp_advantages_run(e))) return rc;
    return pq_update_run(e, epochs, stats_m);
}
