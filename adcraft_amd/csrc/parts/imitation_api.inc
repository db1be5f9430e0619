// imitation_api.inc - the extern "C" entry points of imitation learning (include/adcraft_engine.h; the kernels are
// parts/kernel_imitation.inc, the law csrc/adc_imitation.h): teacher days - days on which an expert acts and the record keeps what
// the learner would have seen next to what the expert did -, DAgger days - teacher days on which a per-env coin picks whose action
// the step consumes (csrc/adc_dagger.h) - and behaviour cloning / MARWIL over such a record as an add-on to the single-learner
// policy-gradient trainer, whose theta, Adam moments, scratch and update kernels it shares (parts/pg_core.inc).
// (part of the single translation unit adc_engine.hip)
namespace {
// the first two steps of a labelled day (a teacher day or a DAgger day; the callers have checked everything):
// 1. the learner's act on the observation the last step left; its bids and budget go to the scratch, the slot takes obs and value
int teach_learner_act(adc_engine *e, float budget)
{
    const int t = e->ro_t, K = e->v.K;
    float *sbids = e->teach_act, *sbudget = e->teach_act + (size_t)e->v.N * (size_t)K;
    return launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *, float *d_budget) {
        const size_t e0 = (size_t)(d_budget - e->d_budget);       // (the group's first env)
        mlp_launch_kernel(v, mlp_view_from(e, e0), st, 0, nullptr, budget, sbids + e0 * (size_t)K, sbudget + e0, rollout_slot(e, true, t, e0), nullptr);
    });
}
// 2. the teacher's act, as one_day has it act (ADC_POLICY_FIXED_ACTIONS: the action buffers as they are)
int teach_teacher_act(adc_engine *e, int teacher, float budget)
{
    int rc;
    if (teacher == ADC_POLICY_ZERO_MARGIN) {
        if ((rc = agent_step_chained(e, budget))) return rc;
        if (e->have_curves && (rc = ideal_step_chained(e))) return rc;
    } else if (teacher == ADC_POLICY_INTERPOLATION) {
        if ((rc = interp_step_chained(e, budget))) return rc;
        if (e->have_curves && (rc = ideal_step_chained(e))) return rc;
    } else if (teacher == ADC_POLICY_ORACLE) {
        if ((rc = ideal_step_chained(e))) return rc;
        if ((rc = policy_oracle_chained(e, budget))) return rc;
    }
    return ADC_OK;
}
// (a day recorded after the envs moved outside the record does not follow the unstored day before it: as mlp_day)
void teach_gap_note(adc_engine *e)
{
    if ((e->have_td3 || e->have_td3_pop || e->have_sac || e->have_sac_pop) && e->ro_t > e->td3_stored_t && e->env_moves != e->ro_moves) e->td3_gap = true;
}

// one teacher day: the learner's act with its action thrown away, the teacher's act, the teacher's action into the record, the
// step, the outcome.  Chained and group-compatible like mlp_day (the callers have checked everything)
int teach_day(adc_engine *e, int teacher, float budget)
{
    const int t = e->ro_t, K = e->v.K;
    int rc;
    teach_gap_note(e);
    if ((rc = teach_learner_act(e, budget)) || (rc = teach_teacher_act(e, teacher, budget))) return rc;
    // 3. the action the step is about to consume into the slot, logp = +0
    if ((rc = launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
            const size_t row = (size_t)t * (size_t)e->v.N + (size_t)(d_budget - e->d_budget);
            const long long lanes = (long long)v.N * (K + 1);
            if (e->mp.bd_lo)            // (the bounded act: the teacher's action in units of the box)
                hipLaunchKernelGGL(k_teach_record_bounded, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, v.N, K, d_bids, d_budget, e->mlp_bd,
                                   e->mlp_bd + 2 * (size_t)(K + 1), e->ro_action + row * (size_t)(K + 1), e->ro_logp + row);
            else
                hipLaunchKernelGGL(k_teach_record, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, v.N, K, d_bids, d_budget,
                                   e->ro_action + row * (size_t)(K + 1), e->ro_logp + row);
        })))
        return rc;
    // 4. the step and the outcome
    if ((rc = launch_step(e, e->d_bids, e->d_budget, nullptr, /* lazy_join = */ true))) return rc;
    if ((rc = mlp_record_outcome_chained(e))) return rc;
    e->ro_teacher += 1;
    return e->es_accumulate ? es_accumulate_chained(e) : ADC_OK;
}

// one DAgger day (adc_dagger.h): both agents act on the same observation, the record keeps the teacher's action as the label, a
// per-env coin picks whose action the step consumes - the scratch, the teacher's action copied over the learner's where the coin
// says so.  The engine's action buffers are left holding the teacher's action.  Chained and group-compatible as teach_day is
int dagger_day(adc_engine *e, int teacher, float budget, float beta)
{
    const int t = e->ro_t, K = e->v.K;
    int rc;
    teach_gap_note(e);
    if ((rc = teach_learner_act(e, budget)) || (rc = teach_teacher_act(e, teacher, budget))) return rc;
    // 3. the label, the played action, the mask
    float *sbids = e->teach_act, *sbudget = e->teach_act + (size_t)e->v.N * (size_t)K;
    const uint64_t threshold = adc::bernoulli_threshold(beta);
    if ((rc = launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
            const size_t e0 = (size_t)(d_budget - e->d_budget), row = (size_t)t * (size_t)e->v.N + e0;
            const long long lanes = (long long)v.N * (K + 1);
            const DaggerMix d{e->mp.key + e0, e->mp.tick + e0, threshold, d_bids, d_budget, sbids + e0 * (size_t)K, sbudget + e0,
                              e->ro_action + row * (size_t)(K + 1), e->ro_logp + row, e->dg_mask + row};
            if (e->mp.bd_lo)            // (the bounded act: the label in units of the box)
                hipLaunchKernelGGL(k_dagger_mix_bounded, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, v.N, K, d, e->mlp_bd,
                                   e->mlp_bd + 2 * (size_t)(K + 1));
            else
                hipLaunchKernelGGL(k_dagger_mix, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, v.N, K, d);
        })))
        return rc;
    // 4. the step consumes the scratch; the outcome
    if ((rc = launch_step(e, sbids, sbudget, nullptr, /* lazy_join = */ true))) return rc;
    if ((rc = mlp_record_outcome_chained(e))) return rc;
    e->dg_day[(size_t)t] = 1;
    e->ro_teacher += 1;
    e->ro_dagger += 1;
    return e->es_accumulate ? es_accumulate_chained(e) : ADC_OK;
}

// what a call of labelled days opens with, behind its own first checks: adc_engine_teach_days' refusals in their order
int teach_enter(const adc_engine *e, int teacher_policy, int32_t days)
{
    if (teacher_policy == ADC_POLICY_MLP) return fail(ADC_EINVAL, "the learned agent cannot be its own teacher: its days are adc_engine_run_days(ADC_POLICY_MLP)");
    if (teacher_policy != ADC_POLICY_FIXED_ACTIONS && teacher_policy != ADC_POLICY_ZERO_MARGIN && teacher_policy != ADC_POLICY_ORACLE &&
        teacher_policy != ADC_POLICY_INTERPOLATION)
        return fail(ADC_EINVAL, "unknown policy");
    if (int rc = mlp_ready(e)) return rc;
    if (int rc = gru_refuses(e, "a teacher's or a DAgger day")) return rc;
    if (e->pop_M != 0) return fail(ADC_ESTATE, "teacher days with a population active are not supported (adc_engine_mlp_population(0) first)");
    if (e->lrn_M != 0) return fail(ADC_ESTATE, "teacher days with learners active are not supported (adc_engine_mlp_learners(0) first)");
    if (e->mp.sq_lo) return fail(ADC_ESTATE, "teacher days under a squashed action are not supported: the record would need the pre-squash action of the teacher");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "teacher days need a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "teacher days need the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    if (days < 0) return fail(ADC_EINVAL, "days < 0");
    if (days > 0 && !rollout_room(e, days)) return fail(ADC_EINVAL, "the rollout record would overflow within these days: adc_engine_rollout_reset first");
    if (teacher_policy == ADC_POLICY_ZERO_MARGIN && !e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    if (teacher_policy == ADC_POLICY_INTERPOLATION) {
        if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
        if (days > 0 && !interp_room(e, days)) return fail(ADC_EINVAL, "the interpolation agent's capacity would overflow within these days");
    }
    if (teacher_policy == ADC_POLICY_ORACLE && !e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    return ADC_OK;
}
// the scratch the learner's bids and budgets of a labelled day go to, allocated at the first such day
int teach_scratch(adc_engine *e)
{
    if (e->teach_act) return ADC_OK;
    if (int rc = mlp_alloc(e, e->teach_allocs, &e->teach_act, (size_t)e->v.N * ((size_t)e->v.K + 1u))) {
        mlp_free(e, e->teach_allocs);
        e->teach_act = nullptr;
        return rc;
    }
    return ADC_OK;
}

int im_ready(const adc_engine *e)
{
    if (!e->have_im) return fail(ADC_ESTATE, "adc_engine_im_init has not been called (or the trainer it lived on has gone)");
    return ADC_OK;
}
// the add-ons and normalisers imitation does not run under (checked at init and again at every call)
int im_addon_check(const adc_engine *e)
{
    if (e->kl_live) return fail(ADC_ESTATE, "the KL penalty is alive on this trainer: imitation has no collecting distribution to penalise against");
    if (e->sh_live) return fail(ADC_ESTATE, "shuffled minibatches are alive on this trainer: imitation updates run over contiguous env minibatches");
    if (e->on.live || e->rn.live) return fail(ADC_ESTATE, "a running normaliser is alive: imitation runs under the static normalisation and unnormalised returns");
    return ADC_OK;
}
// the preamble of the calls that work on the record
int im_enter(const adc_engine *e, int epochs = 1)
{
    int rc;
    if ((rc = im_ready(e)) || (rc = pg_ready(e, false)) || (rc = pg_state_check(e, false)) || (rc = im_addon_check(e))) return rc;
    if (e->ro_t == 0) return fail(ADC_ESTATE, "no day has been recorded (adc_engine_teach_days)");
    if (e->ro_teacher != e->ro_t) return fail(ADC_ESTATE, "the record holds days the learner collected: imitation needs the teacher's action (adc_engine_rollout_reset, adc_engine_teach_days)");
    if (e->ro_dagger > 0 && e->im_cfg.beta != 0.0f)
        return fail(ADC_ESTATE, "the record holds DAgger days: MARWIL's weight needs returns that follow the labelled action, and a DAgger day's follow the "
                                "mixture that drove it (adc_engine_im_init with beta = 0 clones them)");
    if (epochs < 1 || epochs > 65536) return fail(ADC_EINVAL, "epochs: 1 to 65536");
    return ADC_OK;
}
int im_adv_check(const adc_engine *e)
{
    if (!e->im_adv_ready) return fail(ADC_ESTATE, "adc_engine_im_advantages has not been called since the last recorded day");
    return ADC_OK;
}
void im_stats_fill(adc_im_stats *stats, const adc::PgStatsOut &o, int64_t steps, int64_t samples)
{
    stats->steps = steps; stats->samples = samples;
    stats->policy_loss = o.policy_loss; stats->value_loss = o.value_loss; stats->entropy = o.entropy; stats->logp = o.approx_kl;
    stats->weight = o.clip_fraction; stats->grad_norm = o.grad_norm; stats->explained_variance = o.explained_variance;
}

// One gradient of the imitation loss and one step over the recorded days of the envs [n0, n0 + B): k_im_sample, then the
// policy-gradient trainer's weight gradient, sums, norm clip and update as pg_minibatch_run launches them for a single learner
int im_minibatch_run(adc_engine *e, int n0, int B, adc::PgStatsOut *out)
{
    const adc::PgShape &sh = e->pg_shape;
    const int N = e->v.N, nd = adc::pg_deltas_floats(sh), Q = e->pg_lay.Q;
    const long long S = (long long)e->ro_t * B;
    const unsigned chunks = (unsigned)pg_chunks(S);
    PgView p = pg_view_of(e, n0, B);
    p.loss = adc::PgLoss{0.0f, e->im_cfg.vf_coef, 0.0f};
    const adc::ImLaw law{e->im_cfg.beta, e->im_c, e->im_cfg.w_max, e->im_cfg.train_log_std != 0 ? 1 : 0};
    const size_t lds = pg_lds_floats(sh, e->pg_maxw, false) * sizeof(float);
    const dim3 blk(kPgBlock);
    hipLaunchKernelGGL(k_im_sample, dim3((unsigned)S), blk, lds, e->stream, p, law);
    pg_terms_walk(sh, e->ro_obs, e->pg_acts, p.na, [&](const PgTerm &t, unsigned tiles) {
        hipLaunchKernelGGL(k_pg_wgrad, dim3(tiles, chunks), blk, 0, e->stream, t, S, B, N, n0, e->pg_deltas, nd, e->pg_gpart, Q);
    });
    hipLaunchKernelGGL(k_pg_grad_join, dim3(pg_blocks(Q)), blk, 0, e->stream, e->pg_gpart, (int)chunks, Q, S, e->pg_grad);
    HIP_TRY(hipGetLastError());
    int rc;
    if ((rc = pg_csum_launch(e, e->pg_pieces, S, adc::kPgPieces, 7, 0, 0.0, e->pg_sums)) ||
        (rc = pg_csum_launch(e, e->pg_pieces + adc::kPgRet, S, adc::kPgPieces, 2, 2, 0.0, e->pg_sums + 7)) ||
        (rc = pg_csum_launch(e, e->pg_grad, Q, 1, 1, 2, 0.0, e->pg_sums + 9)))
        return rc;
    double sums[adc::kPgSums];
    HIP_TRY(hipMemcpyAsync(sums, e->pg_sums, sizeof(sums), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const adc_pg_config &c = e->pgp_cfg[0];
    const adc::PgStatsOut st = adc::pg_stats_finish(sums, S);
    if (out) *out = st;
    const bool clip = c.max_grad_norm > 0.0f;
    const float scale = clip ? adc::pg_clip_scale(c.max_grad_norm, st.grad_norm) : 1.0f;
    hipLaunchKernelGGL(k_pg_update, dim3(pg_blocks(Q)), blk, 0, e->stream, e->pg_lay, e->pg_theta, e->pg_m, e->pg_v, e->pg_grad, clip ? 1 : 0, scale,
                       pg_step_of(c, e->pgp_steps[0]));
    HIP_TRY(hipGetLastError());
    e->pgp_steps[0] += 1;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_teach_days(adc_engine *e, int teacher_policy, int32_t days, float budget)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (int rc = teach_enter(e, teacher_policy, days)) return rc;
    ENGINE_GUARD(e);
    int rc;
    if ((rc = teach_scratch(e))) return rc;
    for (int d = 0; d < days; ++d)
        if ((rc = teach_day(e, teacher_policy, budget))) return rc;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_dagger_days(adc_engine *e, int teacher_policy, int32_t days, float budget, float beta)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!(beta >= 0.0f && beta <= 1.0f)) return fail(ADC_EINVAL, "beta: the share of envs the teacher drives, in [0, 1]");
    if (teacher_policy == ADC_POLICY_INTERPOLATION)
        return fail(ADC_EINVAL, "the interpolation agent cannot teach a DAgger day: its update keys its points by the bid it returned, which on a "
                                "learner-driven day is not the bid the outcomes came from (adc_engine_teach_days takes it)");
    if (int rc = teach_enter(e, teacher_policy, days)) return rc;
    ENGINE_GUARD(e);
    int rc;
    if ((rc = teach_scratch(e))) return rc;
    if (!e->dg_mask) {                  // (the mask: the record's allocation, gone with it)
        if ((rc = mlp_alloc(e, e->ro_allocs, &e->dg_mask, (size_t)e->ro_T * (size_t)e->v.N))) return rc;
        e->dg_day.assign((size_t)e->ro_T, (uint8_t)0);
    }
    for (int d = 0; d < days; ++d)
        if ((rc = dagger_day(e, teacher_policy, budget, beta))) return rc;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_dagger_mask_fetch(adc_engine *e, uint8_t *out_tn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!out_tn) return fail(ADC_EINVAL, "out_tn is NULL");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "adc_engine_rollout_enable has not been called");
    if (e->ro_teacher != e->ro_t) return fail(ADC_ESTATE, "the record holds days the learner collected: they have no teacher and no mask (adc_engine_rollout_reset)");
    ENGINE_GUARD(e);
    const size_t N = (size_t)e->v.N;
    if (e->ro_dagger > 0) {
        HIP_TRY(hipMemcpyAsync(out_tn, e->dg_mask, (size_t)e->ro_t * N, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    for (int t = 0; t < e->ro_t; ++t)       // (a plain teacher day: the teacher drove every env)
        if (e->ro_dagger == 0 || !e->dg_day[(size_t)t]) std::memset(out_tn + (size_t)t * N, 1, N);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_im_init(adc_engine *e, const adc_im_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_im_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = gru_refuses(e, "imitation learning")) return rc;
    if (e->have_pg_pop) return fail(ADC_ESTATE, "imitation is an add-on to a single-learner trainer: a learner population is alive (adc_engine_pg_init)");
    if (!e->have_pg) return fail(ADC_ESTATE, "imitation is an add-on to a single-learner PPO / A2C trainer: adc_engine_pg_init first");
    int rc;
    if ((rc = pg_state_check(e, false)) || (rc = im_addon_check(e))) return rc;
    if ((rc = pg_lds_refuse(e, e->pg_shape, e->pg_maxw, false))) return rc;
    ENGINE_GUARD(e);
    e->im_cfg = *cfg;
    e->im_ma = cfg->ma_start;
    e->im_calls = 0;
    e->im_c = 0.0f;
    e->im_adv_ready = false;
    e->have_im = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_im_advantages(adc_engine *e, float *adv_tn, float *ret_tn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = im_enter(e)) return rc;
    ENGINE_GUARD(e);
    const int N = e->v.N, T = e->ro_t;
    const long long tn = (long long)T * N;
    const adc_pg_config &c = e->pgp_cfg[0];
    int rc;
    if ((rc = pg_boot_launch(e))) return rc;
    hipLaunchKernelGGL(k_pg_gae, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, N, T, e->ro_reward, e->ro_term, e->ro_trunc, e->ro_value, e->mlp_boot,
                       c.gamma, c.gamma * 1.0f, c.reward_scale, e->pg_adv, e->pg_ret);
    HIP_TRY(hipGetLastError());
    double sumsq = 0.0;
    if ((rc = pg_csum_launch(e, e->pg_adv, tn, 1, 1, 2, 0.0, e->pg_sums))) return rc;
    HIP_TRY(hipMemcpyAsync(&sumsq, e->pg_sums, 8, hipMemcpyDeviceToHost, e->stream));
    const size_t bytes = (size_t)tn * 4;
    if (adv_tn) HIP_TRY(hipMemcpyAsync(adv_tn, e->pg_adv, bytes, hipMemcpyDeviceToHost, e->stream));
    if (ret_tn) HIP_TRY(hipMemcpyAsync(ret_tn, e->pg_ret, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->im_ma = adc::im_ma_next(e->im_ma, e->im_cfg.ma_rate, sumsq, tn, e->im_c);
    e->im_calls += 1;
    e->pg_adv_ready = false;            // (pg_adv / pg_ret now hold the teacher's returns, not an on-policy update's advantages)
    e->im_adv_ready = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_im_minibatch(adc_engine *e, int32_t env_begin, int32_t env_count, adc_im_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = im_enter(e)) || (rc = im_adv_check(e))) return rc;
    if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > e->v.N) return fail(ADC_EINVAL, "the env range is not inside [0, num_envs)");
    if (env_count > e->pg_mb) return fail(ADC_EINVAL, "env_count exceeds the configuration's minibatch_envs (the scratch was sized for it)");
    ENGINE_GUARD(e);
    adc::PgStatsOut o;
    if ((rc = im_minibatch_run(e, env_begin, env_count, &o))) return rc;
    if (stats) im_stats_fill(stats, o, e->pgp_steps[0], (int64_t)e->ro_t * env_count);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_im_update(adc_engine *e, int32_t epochs, adc_im_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = im_enter(e, epochs)) || (rc = im_adv_check(e))) return rc;
    ENGINE_GUARD(e);
    const int mb = e->pg_mb, count = e->v.N / mb;
    adc::PgStatsOut o, acc, mean{};
    for (int ep = 0; ep < epochs; ++ep) {
        acc = adc::PgStatsOut{};
        for (int i = 0; i < count; ++i) {
            if ((rc = im_minibatch_run(e, i * mb, mb, &o))) return rc;
            pg_stats_add(acc, o);
        }
        mean = pg_stats_mean(acc, count);
    }
    if (stats) im_stats_fill(stats, mean, e->pgp_steps[0], (int64_t)e->ro_t * mb);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_im_state_get(adc_engine *e, double *ma, int64_t *calls)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = im_ready(e)) return rc;
    if (ma) *ma = e->im_ma;
    if (calls) *calls = e->im_calls;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_im_state_set(adc_engine *e, double ma, int64_t calls)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = im_ready(e)) return rc;
    if (!(ma >= 0.0) || !std::isfinite(ma)) return fail(ADC_EINVAL, "ma: finite and >= 0");
    if (calls < 0) return fail(ADC_EINVAL, "calls >= 0");
    e->im_ma = ma;
    e->im_calls = calls;
    e->im_adv_ready = false;            // (the scale of the last advantages call belonged to the old state)
    return ADC_OK;
}
