// pbt_api.inc - the extern "C" entry points of the population-based training scheduler (include/adcraft_engine.h; the kernels are
// parts/kernel_pbt.inc, the law csrc/adc_pbt.h) over the live learner population: adc_engine_pg_pop_* (parts/pg_api.inc),
// adc_engine_td3_pop_* (parts/td3_pop_api.inc) or adc_engine_sac_pop_* (parts/sac_pop_api.inc; adc_engine_pbt_init_sac).  The
// members' configurations are host-mastered there (pgp_cfg / tp_cfg / sp_cfg and the member tables made from them), so the plan -
// ranking, donor draw, explored values - runs on the host from the M doubles of the fitness, with the law header's own functions;
// what is per replaced member on the device is one (dst, src) table.
// A round's launches and host round trips, whatever M and replace_count (read from this code, not from a trace):
//   fitness   1 launch (k_pbt_fitness), 1 copy of M doubles down, 1 wait - or, with a fitness handed in, the wait alone (an
//             upload of the host's member table may still be in flight);
//   exploit   1 copy of the pair table up; PG: 1 launch; TD3: 4 launches (actor, critics, target actor, target critics; the
//             actor's also writes the explored log_std), and 1 more for the five ring arrays with with_ring; SAC: 4 launches
//             (actor, critics, target critics - there is no target actor - and k_pbt_exploit_cell: the temperature cells, copied
//             or explored), and 1 more for the ring with with_ring;
//   explore   1 copy of the member table up (SAC: 2, its two member tables);
//   then      1 wait.
// So a round's host waits are 2 for every kind - one before the plan (the fitness fetch's, or the one in front of the host
// tables' writes), one at the end - and adc_engine_pbt_exploit's are 2 as well (one in front, one at the end).
// (part of the single translation unit adc_engine.hip)
namespace {
int pbt_ready(const adc_engine *e)
{
    if (!e->have_pbt)
        return fail(ADC_ESTATE, "adc_engine_pbt_init / adc_engine_pbt_init_sac has not been called (or the population trainer under it, the learners, the policy or the record were re-initialised since)");
    return ADC_OK;
}
// a member's hyperparameters by id, from and into its host-mastered configuration (TD3's sigma is not there: the device's log_std)
void pbt_hp_get(const adc_engine *e, int m, float hp[adc::kPbtMaxHp])
{
    for (int h = 0; h < adc::kPbtMaxHp; ++h) hp[h] = 0.0f;
    if (e->pbt_kind == ADC_PBT_PG) {
        const adc_pg_config &c = e->pgp_cfg[(size_t)m];
        hp[0] = c.lr; hp[1] = c.ent_coef; hp[2] = c.eps_clip; hp[3] = c.vf_coef;
    } else if (e->pbt_kind == ADC_PBT_SAC) {
        const adc_sac_config &c = e->sp_cfg[(size_t)m];
        hp[0] = c.actor_lr; hp[1] = c.critic_lr; hp[2] = c.alpha_lr; hp[3] = c.tau; hp[5] = c.target_entropy;
    } else {
        const adc_td3_config &c = e->tp_cfg[(size_t)m];
        hp[0] = c.actor_lr; hp[1] = c.critic_lr; hp[2] = c.target_noise; hp[3] = c.tau;
    }
}
void pbt_hp_put(adc_engine *e, int m, const float hp[adc::kPbtMaxHp])
{
    if (e->pbt_kind == ADC_PBT_PG) {
        adc_pg_config &c = e->pgp_cfg[(size_t)m];
        c.lr = hp[0]; c.ent_coef = hp[1]; c.eps_clip = hp[2]; c.vf_coef = hp[3];
        pgp_member_fill(e->pgp_mem[(size_t)m], c);
    } else if (e->pbt_kind == ADC_PBT_SAC) {
        // (as adc_engine_sac_pop_set_config: sp_cfg, tp_cfg through sac_as_td3, the member's rows of the two tables)
        adc_sac_config &c = e->sp_cfg[(size_t)m];
        c.actor_lr = hp[0]; c.critic_lr = hp[1]; c.alpha_lr = hp[2]; c.tau = hp[3]; c.target_entropy = hp[5];
        e->tp_cfg[(size_t)m] = sac_as_td3(c);
        sp_member_fill(e, (size_t)m, c);
    } else {
        adc_td3_config &c = e->tp_cfg[(size_t)m];
        c.actor_lr = hp[0]; c.critic_lr = hp[1]; c.target_noise = hp[2]; c.tau = hp[3];
        tp_member_fill(e, e->tp_mem[(size_t)m], c);
    }
}
// the five ring arrays of every pair's donor into its destination's, in one launch (TD3 and SAC populations: the members' rings are
// tp_dmem's either way); under n-step returns gn travels as a sixth
void pbt_ring_launch(adc_engine *e, int npairs)
{
    const size_t C = (size_t)e->td3_cfg.capacity, most = C * (size_t)e->td3_shape.D * 4u;
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>((most / 16u + kPbtBlock - 1) / kPbtBlock, 1), 256);
    hipLaunchKernelGGL(k_pbt_exploit_ring, dim3(blocks, (unsigned)npairs, e->nstep_n ? 6u : 5u), dim3(kPbtBlock), 0, e->stream, e->tp_dmem, e->pbt_dpairs, C, e->td3_shape.D,
                       e->td3_shape.A);
}
// the first `npairs` entries of pbt_pairs: up in one copy, then every pair's copy in the same launches
int pbt_exploit_launch(adc_engine *e, int npairs)
{
    if (npairs == 0) return ADC_OK;
    HIP_TRY(hipMemcpyAsync(e->pbt_dpairs, e->pbt_pairs.data(), (size_t)npairs * sizeof(PbtPair), hipMemcpyHostToDevice, e->stream));
    if (e->pbt_kind == ADC_PBT_PG) {
        hipLaunchKernelGGL(k_pbt_exploit, dim3(pg_blocks(e->lrn_lay.Q), (unsigned)npairs), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, e->pg_theta,
                           e->pg_m, e->pg_v, e->pbt_dpairs, (float *)nullptr, (size_t)0, 0, 0.0f, 0.0f);
    } else if (e->pbt_kind == ADC_PBT_SAC) {
        // (the SAC population keeps its vectors, layouts and rings in the TD3 population's fields: the actor's and the critics'
        // vectors with their two moment vectors each, the target critics' with none; no target actor, no log_std to explore)
        for (int w = 0; w < 4; ++w) {
            if (w == kTd3ThetaT) continue;
            const PgLayout &lay = e->td3_lay[w];
            float *mm = w < 2 ? e->td3_mom[2 * w] : nullptr, *mv = w < 2 ? e->td3_mom[2 * w + 1] : nullptr;
            hipLaunchKernelGGL(k_pbt_exploit, dim3(pg_blocks(lay.Q), (unsigned)npairs), dim3(kPgBlock), 0, e->stream, lay, e->tp_stride[w], e->td3_flat[w], mm, mv,
                               e->pbt_dpairs, (float *)nullptr, (size_t)0, 0, 0.0f, 0.0f);
        }
        hipLaunchKernelGGL(k_pbt_exploit_cell, dim3((unsigned)((npairs + kPbtBlock - 1) / kPbtBlock)), dim3(kPbtBlock), 0, e->stream, npairs, e->sp_cells,
                           e->pbt_dpairs, e->pbt_cfg.lo[adc::kPbtAlpha], e->pbt_cfg.hi[adc::kPbtAlpha]);
        if (e->pbt_cfg.with_ring) pbt_ring_launch(e, npairs);
        if (e->pbt_cfg.with_ring && e->per_live) per_pairs_launch(e, npairs);     // (the leaves, nodes and tops travel with the rings)
    } else {
        for (int w = 0; w < 4; ++w) {
            const PgLayout &lay = e->td3_lay[w];
            float *mm = w < 2 ? e->td3_mom[2 * w] : nullptr, *mv = w < 2 ? e->td3_mom[2 * w + 1] : nullptr;
            // (the members' log_std vectors: the learners' last term, as adc_engine_mlp_set_learner_log_std finds them)
            float *ls = w == kTd3Theta ? e->lrn_lay.b[e->lrn_lay.nterms - 1] : nullptr;
            hipLaunchKernelGGL(k_pbt_exploit, dim3(pg_blocks(lay.Q), (unsigned)npairs), dim3(kPgBlock), 0, e->stream, lay, e->tp_stride[w], e->td3_flat[w], mm, mv,
                               e->pbt_dpairs, ls, e->lrn_stride, e->td3_shape.A, e->pbt_cfg.lo[adc::kPbtSigma], e->pbt_cfg.hi[adc::kPbtSigma]);
        }
        if (e->pbt_cfg.with_ring) pbt_ring_launch(e, npairs);
        if (e->pbt_cfg.with_ring && e->per_live) per_pairs_launch(e, npairs);     // (the leaves, nodes and tops travel with the rings)
    }
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// what the host keeps per member follows the donor (a live KL add-on's coefficients are then uploaded by the caller: kl_copy)
void pbt_bookkeeping(adc_engine *e, int npairs)
{
    const size_t per = 2u * adc::kMlpMaxLayers;
    for (int j = 0; j < npairs; ++j) {
        const size_t to = (size_t)e->pbt_pairs[(size_t)j].dst, from = (size_t)e->pbt_pairs[(size_t)j].src;
        if (e->pbt_kind == ADC_PBT_PG) e->pgp_steps[to] = e->pgp_steps[from];
        else
            for (size_t i = 0; i < per; ++i) e->tp_critic_set[to * per + i] = e->tp_critic_set[from * per + i];
    }
}
// the members' fitness from the record: one launch, M doubles down, one wait
int pbt_fitness_run(adc_engine *e, double *fitness_m)
{
    const int M = e->lrn_M;
    hipLaunchKernelGGL(k_pbt_fitness, dim3((unsigned)M), dim3(kPbtBlock), 0, e->stream, e->v.N, e->ro_t, e->lrn_n, e->ro_reward, e->pbt_ret, e->pbt_fit);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e->pbt_host_fit.data(), e->pbt_fit, (size_t)M * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int m = 0; m < M; ++m) fitness_m[m] = e->pbt_host_fit[(size_t)m];
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_pbt_init(adc_engine *e, const adc_pbt_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_pg_pop && !e->have_td3_pop)
        return fail(ADC_ESTATE, "population-based training needs a live population trainer (adc_engine_pg_pop_init or adc_engine_td3_pop_init)");
    const int kind = e->have_pg_pop ? ADC_PBT_PG : ADC_PBT_TD3, M = e->lrn_M;
    const char *why = nullptr;
    if (adc_pbt_config_check(cfg, M, kind, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    ENGINE_GUARD(e);
    if (!e->have_pbt) {
        // (the trainer owns the arrays: they are freed with it, and pg_drop / td3_drop forget the scheduler)
        std::vector<void *> &owner = kind == ADC_PBT_PG ? e->pg_allocs : e->td3_allocs;
        double *ret = nullptr, *fit = nullptr;
        PbtPair *pairs = nullptr;
        int rc;
        if ((rc = mlp_alloc(e, owner, &ret, (size_t)e->v.N)) || (rc = mlp_alloc(e, owner, &fit, (size_t)M)) || (rc = mlp_alloc(e, owner, &pairs, (size_t)M))) return rc;
        e->pbt_ret = ret; e->pbt_fit = fit; e->pbt_dpairs = pairs;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pbt_kind = kind;
    e->pbt_cfg = *cfg;
    e->pbt_key = adc::pbt_key(cfg->seed ? cfg->seed : e->cfg.seed);
    e->pbt_round = 0;
    e->pbt_s.assign((size_t)M, 0.0);
    e->pbt_host_fit.assign((size_t)M, 0.0);
    e->pbt_pairs.assign((size_t)M, PbtPair{});
    e->have_pbt = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pbt_init_sac(adc_engine *e, const adc_pbt_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_sac_pop) return fail(ADC_ESTATE, "population-based training over SAC needs a live SAC population trainer (adc_engine_sac_pop_init)");
    const int M = e->lrn_M;
    const char *why = nullptr;
    if (adc_pbt_config_check(cfg, M, ADC_PBT_SAC, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    ENGINE_GUARD(e);
    if (!e->have_pbt) {
        // (the SAC population's arrays are td3_allocs: they are freed with it, and td3_drop forgets the scheduler)
        double *ret = nullptr, *fit = nullptr;
        PbtPair *pairs = nullptr;
        int rc;
        if ((rc = mlp_alloc(e, e->td3_allocs, &ret, (size_t)e->v.N)) || (rc = mlp_alloc(e, e->td3_allocs, &fit, (size_t)M)) ||
            (rc = mlp_alloc(e, e->td3_allocs, &pairs, (size_t)M)))
            return rc;
        e->pbt_ret = ret; e->pbt_fit = fit; e->pbt_dpairs = pairs;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pbt_kind = ADC_PBT_SAC;
    e->pbt_cfg = *cfg;
    e->pbt_key = adc::pbt_key(cfg->seed ? cfg->seed : e->cfg.seed);
    e->pbt_round = 0;
    e->pbt_s.assign((size_t)M, 0.0);
    e->pbt_host_fit.assign((size_t)M, 0.0);
    e->pbt_pairs.assign((size_t)M, PbtPair{});
    e->have_pbt = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pbt_fitness(adc_engine *e, double *fitness_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pbt_ready(e)) return rc;
    if (!fitness_m) return fail(ADC_EINVAL, "fitness_m is NULL");
    if (e->ro_t == 0) return fail(ADC_ESTATE, "no recorded day (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    ENGINE_GUARD(e);
    return pbt_fitness_run(e, fitness_m);
}

ADC_EXPORT int adc_engine_pbt_exploit(adc_engine *e, const int32_t *src_of_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pbt_ready(e)) return rc;
    if (!src_of_m) return fail(ADC_EINVAL, "src_of_m is NULL");
    const int M = e->lrn_M;
    for (int m = 0; m < M; ++m)
        if (src_of_m[m] < -1 || src_of_m[m] >= M) return fail(ADC_EINVAL, "src_of_m: a member, or the member itself / -1 to keep it");
    for (int m = 0; m < M; ++m) {
        const int s = src_of_m[m];
        if (s == -1 || s == m) continue;
        if (src_of_m[s] != -1 && src_of_m[s] != s) return fail(ADC_EINVAL, "a destination is also a source: the copies of a round may not chain");
    }
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    int npairs = 0;
    for (int m = 0; m < M; ++m)
        if (src_of_m[m] != -1 && src_of_m[m] != m) e->pbt_pairs[(size_t)npairs++] = PbtPair{m, src_of_m[m], 0, 0.0f};
    if (int rc = pbt_exploit_launch(e, npairs)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    pbt_bookkeeping(e, npairs);
    if (e->pbt_kind == ADC_PBT_PG)
        if (int rc = kl_copy(e, npairs, [&](int j, int &d, int &f) { d = e->pbt_pairs[(size_t)j].dst; f = e->pbt_pairs[(size_t)j].src; })) return rc;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pbt_step(adc_engine *e, const double *fitness_m, adc_pbt_result *result_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pbt_ready(e)) return rc;
    if (!fitness_m && e->ro_t == 0) return fail(ADC_ESTATE, "no recorded day to take the fitness from (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    if (e->pbt_round >= 0xFFFFFFFEll) return fail(ADC_ESTATE, "the round counter is exhausted");
    ENGINE_GUARD(e);
    const int M = e->lrn_M, q = e->pbt_cfg.replace_count;
    const adc_pbt_config &cfg = e->pbt_cfg;
    const size_t Ms = (size_t)M;
    int rc;
    // fitness; either way the stream has been waited for before the host's member table is written
    std::vector<double> f(Ms);
    if (fitness_m) {
        f.assign(fitness_m, fitness_m + M);
        HIP_TRY(hipStreamSynchronize(e->stream));
    } else if ((rc = pbt_fitness_run(e, f.data()))) return rc;
    // smoothing and the plan, on the host from M doubles
    for (size_t m = 0; m < Ms; ++m) e->pbt_s[m] = adc::pbt_smooth(cfg.fitness_ema, e->pbt_s[m], f[m], e->pbt_round == 0);
    std::vector<int32_t> rank(Ms), src(Ms);
    std::vector<uint32_t> bits(Ms);
    adc::pbt_plan(e->pbt_key, (uint32_t)e->pbt_round, q, e->pbt_s.data(), M, rank.data(), src.data(), bits.data());
    // the pair table and the explored hyperparameters (donors are never replaced: their values are the round's old ones)
    // (id 4 - TD3's sigma, SAC's alpha - is the device's: the pair carries the log-domain shift, the exploit's launch applies it)
    const bool sigma = (e->pbt_kind == ADC_PBT_TD3 || e->pbt_kind == ADC_PBT_SAC) && ((cfg.tuned_mask >> adc::kPbtSigma) & 1u);
    std::vector<float> shift(Ms, 0.0f);
    int npairs = 0;
    for (int m = 0; m < M; ++m) {
        if (src[(size_t)m] < 0) continue;
        float donor[adc::kPbtMaxHp], own[adc::kPbtMaxHp], out[adc::kPbtMaxHp];
        pbt_hp_get(e, src[(size_t)m], donor);
        pbt_hp_get(e, m, own);
        for (int h = 0; h < adc::kPbtMaxHp; ++h) {
            const bool tuned = ((cfg.tuned_mask >> h) & 1u) && !(e->pbt_kind != ADC_PBT_PG && h == adc::kPbtSigma);
            out[h] = tuned ? adc::pbt_explore(donor[h], (int)((bits[(size_t)m] >> h) & 1u), cfg.factor_lo, cfg.factor_hi, cfg.lo[h], cfg.hi[h]) : own[h];
        }
        pbt_hp_put(e, m, out);
        if (sigma) shift[(size_t)m] = ((bits[(size_t)m] >> adc::kPbtSigma) & 1u) ? cfg.log_factor_hi : cfg.log_factor_lo;
        e->pbt_pairs[(size_t)npairs++] = PbtPair{m, src[(size_t)m], sigma ? 1 : 0, shift[(size_t)m]};
    }
    // exploit: every pair in the same launches; explore: the member table up in one copy
    if ((rc = pbt_exploit_launch(e, npairs))) return rc;
    if ((rc = e->pbt_kind == ADC_PBT_PG ? pgp_members_upload(e) : e->pbt_kind == ADC_PBT_SAC ? sp_members_upload(e) : tp_members_upload(e))) return rc;
    if (e->pbt_kind == ADC_PBT_PG) e->pg_adv_ready = false;       // (as adc_engine_pg_pop_set_config leaves it)
    pbt_bookkeeping(e, npairs);
    if (e->pbt_kind == ADC_PBT_PG && (rc = kl_copy(e, npairs, [&](int j, int &d, int &f) { d = e->pbt_pairs[(size_t)j].dst; f = e->pbt_pairs[(size_t)j].src; })))
        return rc;
    for (int j = 0; j < npairs; ++j) e->pbt_s[(size_t)e->pbt_pairs[(size_t)j].dst] = e->pbt_s[(size_t)e->pbt_pairs[(size_t)j].src];
    e->pbt_round += 1;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (result_m)
        for (int m = 0; m < M; ++m) {
            adc_pbt_result &r = result_m[m];
            r.fitness = f[(size_t)m]; r.smoothed = e->pbt_s[(size_t)m]; r.rank = rank[(size_t)m]; r.src = src[(size_t)m];
            pbt_hp_get(e, m, r.hp);
            if (e->pbt_kind != ADC_PBT_PG) r.hp[adc::kPbtSigma] = shift[(size_t)m];
        }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pbt_state_get(adc_engine *e, int64_t *round, double *smoothed_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pbt_ready(e)) return rc;
    if (round) *round = e->pbt_round;
    if (smoothed_m)
        for (int m = 0; m < e->lrn_M; ++m) smoothed_m[m] = e->pbt_s[(size_t)m];
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pbt_state_set(adc_engine *e, int64_t round, const double *smoothed_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = pbt_ready(e)) return rc;
    if (!smoothed_m) return fail(ADC_EINVAL, "smoothed_m is NULL");
    if (round < 0 || round >= 0xFFFFFFFEll) return fail(ADC_EINVAL, "round: 0 to 2^32 - 3");
    e->pbt_round = round;
    e->pbt_s.assign(smoothed_m, smoothed_m + e->lrn_M);
    return ADC_OK;
}
