// pg_kl_api.inc - the extern "C" entry points of the PPO learners' KL penalty and value-loss clip (include/adcraft_engine.h; the
// kernels are parts/kernel_pg_kl.inc, the law csrc/adc_pg_kl.h), and what parts/pg_api.inc calls of the add-on: the snapshot at
// the advantages, the sample pass under it, the statistics and the adaptation.  The coefficients are host-mastered (kl_coef): a
// single learner's is a kernel argument, a population's members' are one small table on the device, uploaded when they change -
// after an update's adaptation, a copy or adc_engine_pg_kl_coef_set - in ONE copy whatever M is.
// (part of the single translation unit adc_engine.hip)
namespace {
constexpr const char *kKlNotReady =
    "adc_engine_pg_kl_init has not been called (or the trainer, the policy, the learners or the record were re-initialised since)";

// the members' table from the host's coefficients and configurations, up in one copy (a population's; a single learner has none)
// (idle: the caller has waited for the stream since the last upload - the queued update's one wait)
int kl_members_upload(adc_engine *e, bool idle = false)
{
    if (!e->have_pg_pop) return ADC_OK;
    if (!idle) HIP_TRY(hipStreamSynchronize(e->stream));       // (an earlier upload of the host's table may still be in flight)
    for (size_t m = 0; m < e->kl_mem.size(); ++m) e->kl_mem[m].kl = adc::PgKl{e->kl_coef[m], e->kl_cfg[m].vf_clip};
    HIP_TRY(hipMemcpyAsync(e->kl_dmem, e->kl_mem.data(), e->kl_mem.size() * sizeof(PgKlMember), hipMemcpyHostToDevice, e->stream));
    return ADC_OK;
}

// the collecting distribution of every recorded row under the parameters in force now (the advantages calls, while the add-on lives)
int kl_snapshot_launch(adc_engine *e)
{
    const adc::PgShape &sh = e->pg_shape;
    const size_t rows = (size_t)e->ro_t * (size_t)e->v.N, lds = pg_old_lds_floats(sh) * sizeof(float);
    if (e->have_pg_pop)
        hipLaunchKernelGGL(k_pg_pop_old_dist, dim3((unsigned)rows), dim3(kPgBlock), lds, e->stream, sh, e->lrn_tab, e->v.N, e->lrn_n, e->lrn_M, e->ro_obs,
                           e->kl_mean_old, e->kl_ls_old);
    else
        hipLaunchKernelGGL(k_pg_old_dist, dim3((unsigned)rows), dim3(kPgBlock), lds, e->stream, sh, e->mp.pol, e->mp.log_std, e->ro_obs, e->kl_mean_old,
                           e->kl_ls_old);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

PgKlView kl_view(const adc_engine *e) { return PgKlView{e->kl_mean_old, e->kl_ls_old, e->pg_shape.two_heads, e->kl_pieces}; }

// member m's statistics of a minibatch from its two sums (pg_sums[m * 16 + 10 ...]) over S samples
void kl_stats_minibatch(adc_engine *e, int m, const double *sums2, long long S)
{
    adc_pg_kl_stats &st = e->kl_stats[(size_t)m];
    st.kl = sums2[adc::kPgKlKl] / (double)S;
    st.vf_clip_fraction = sums2[adc::kPgKlVfClipped] / (double)S;
    st.kl_coef = st.kl_coef_next = e->kl_coef[(size_t)m];
}

// an update's running means of the members' minibatch statistics, and its end: the last epoch's means, the adaptation
// (live: under shuffled minibatches, the members whose update has not stopped - a stopped member keeps the sums and the count of
//  the last epoch it began; NULL: all members)
struct KlEpoch {
    std::vector<double> kl, frac;
    std::vector<int> n;
    void begin(const adc_engine *e, const uint8_t *live = nullptr)
    {
        const size_t M = e->kl_stats.size();
        kl.resize(M, 0.0); frac.resize(M, 0.0); n.resize(M, 0);
        for (size_t m = 0; m < M; ++m)
            if (!live || live[m]) { kl[m] = 0.0; frac[m] = 0.0; n[m] = 0; }
    }
    void add(const adc_engine *e, const uint8_t *live = nullptr)
    {
        for (size_t m = 0; m < kl.size(); ++m)
            if (!live || live[m]) { kl[m] = kl[m] + e->kl_stats[m].kl; frac[m] = frac[m] + e->kl_stats[m].vf_clip_fraction; n[m] += 1; }
    }
};
int kl_update_end(adc_engine *e, const KlEpoch &last, bool idle = false)
{
    bool changed = false;
    for (size_t m = 0; m < e->kl_stats.size(); ++m) {
        adc_pg_kl_stats &st = e->kl_stats[m];
        st.kl = last.kl[m] / (double)last.n[m];
        st.vf_clip_fraction = last.frac[m] / (double)last.n[m];
        st.kl_coef = e->kl_coef[m];
        st.kl_coef_next = adc::pg_kl_adapt(adc::pg_kl_adapt_of(e->kl_cfg[m]), e->kl_coef[m], st.kl);
        changed = changed || st.kl_coef_next != e->kl_coef[m];
        e->kl_coef[m] = st.kl_coef_next;
    }
    return changed ? kl_members_upload(e, idle) : ADC_OK;
}

// dst takes its donors' coefficients (adc_engine_pg_pop_copy, a PBT round's copy): pairs of (dst, src), then one upload
template <class Pairs>
int kl_copy(adc_engine *e, int npairs, Pairs pair)
{
    if (!e->kl_live || npairs == 0) return ADC_OK;
    for (int j = 0; j < npairs; ++j) {
        int dst, src;
        pair(j, dst, src);
        e->kl_coef[(size_t)dst] = e->kl_coef[(size_t)src];
    }
    return kl_members_upload(e);
}
}  // namespace

ADC_EXPORT int adc_engine_pg_kl_init(adc_engine *e, const adc_pg_kl_config *cfgs, int32_t count)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (e->have_td3 || e->have_td3_pop) return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: the KL penalty belongs to the PPO / A2C loss");
    if (!e->have_pg && !e->have_pg_pop)
        return fail(ADC_ESTATE, "the KL penalty is an add-on to a PPO / A2C trainer: adc_engine_pg_init or adc_engine_pg_pop_init first");
    if (e->have_im) return fail(ADC_ESTATE, "imitation is alive on this trainer (adc_engine_im_init): its loss has no collecting distribution to penalise against");
    const int M = pg_members(e);
    if (!cfgs) return fail(ADC_EINVAL, "adc_pg_kl_config array is NULL");
    if (count != 1 && count != M) return fail(ADC_EINVAL, "count: 1 (one configuration shared by all members) or the number of members");
    for (int i = 0; i < count; ++i) {
        const char *why = nullptr;
        if (adc_pg_kl_config_check(cfgs + i, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    }
    const adc::PgShape &sh = e->pg_shape;
    if (int rc = pg_lds_refuse(e, sh, e->pg_maxw, true)) return rc;
    const size_t tna = (size_t)e->ro_T * (size_t)e->v.N * (size_t)sh.A;
    if ((size_t)e->ro_T * (size_t)e->v.N > 0x7FFFFFFFull) return fail(ADC_EINVAL, "horizon x num_envs: at most 2^31 - 1 recorded rows under the KL penalty");
    ENGINE_GUARD(e);
    if (!e->kl_mean_old) {
        // (the trainer owns the arrays: they are freed with it, and pg_drop forgets the add-on; a second init reuses them)
        float *mean_old = nullptr, *ls_old = nullptr, *pieces = nullptr;
        PgKlMember *dmem = nullptr;
        int rc;
        if ((rc = mlp_alloc(e, e->pg_allocs, &mean_old, tna)) || (rc = mlp_alloc(e, e->pg_allocs, &ls_old, sh.two_heads ? tna : (size_t)M * (size_t)sh.A)) ||
            (rc = mlp_alloc(e, e->pg_allocs, &pieces, (size_t)M * e->pg_slots * (size_t)adc::kPgKlPieces)) ||
            (rc = mlp_alloc(e, e->pg_allocs, &dmem, (size_t)M)))
            return rc;
        e->kl_mean_old = mean_old; e->kl_ls_old = ls_old; e->kl_pieces = pieces; e->kl_dmem = dmem;
    }
    e->kl_cfg.assign((size_t)M, cfgs[0]);
    if (count > 1) e->kl_cfg.assign(cfgs, cfgs + M);
    e->kl_coef.resize((size_t)M);
    for (size_t m = 0; m < (size_t)M; ++m) e->kl_coef[m] = e->kl_cfg[m].kl_coef;
    e->kl_stats.assign((size_t)M, adc_pg_kl_stats{});
    for (size_t m = 0; m < (size_t)M; ++m) e->kl_stats[m].kl_coef = e->kl_stats[m].kl_coef_next = e->kl_coef[m];
    e->kl_mem.assign((size_t)M, PgKlMember{});
    e->kl_live = true;
    if (int rc = kl_members_upload(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pg_adv_ready = false;            // (a minibatch needs the snapshot the next advantages call takes)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_kl_stats(adc_engine *e, adc_pg_kl_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->kl_live) return fail(ADC_ESTATE, kKlNotReady);
    if (!stats_m) return fail(ADC_EINVAL, "stats_m is NULL");
    std::copy(e->kl_stats.begin(), e->kl_stats.end(), stats_m);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_kl_coef_get(adc_engine *e, int32_t member, float *coef)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->kl_live) return fail(ADC_ESTATE, kKlNotReady);
    if (member < 0 || member >= pg_members(e)) return fail(ADC_EINVAL, "no such member");
    if (!coef) return fail(ADC_EINVAL, "coef is NULL");
    *coef = e->kl_coef[(size_t)member];
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_kl_coef_set(adc_engine *e, int32_t member, float coef)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->kl_live) return fail(ADC_ESTATE, kKlNotReady);
    if (member < 0 || member >= pg_members(e)) return fail(ADC_EINVAL, "no such member");
    if (!(coef >= 0.0f && coef < __builtin_inff())) return fail(ADC_EINVAL, "coef >= 0 and finite");
    ENGINE_GUARD(e);
    e->kl_coef[(size_t)member] = coef;
    e->kl_stats[(size_t)member].kl_coef_next = coef;
    if (int rc = kl_members_upload(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_kl_old_dist_fetch(adc_engine *e, float *mean_old_tna, float *ls_old)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->kl_live) return fail(ADC_ESTATE, kKlNotReady);
    if (!e->pg_adv_ready) return fail(ADC_ESTATE, "the advantages (and with them the snapshot) have not been computed since the last recorded day");
    ENGINE_GUARD(e);
    const size_t A = (size_t)e->pg_shape.A, tna = (size_t)e->ro_t * (size_t)e->v.N * A;
    if (mean_old_tna) HIP_TRY(hipMemcpyAsync(mean_old_tna, e->kl_mean_old, tna * 4, hipMemcpyDeviceToHost, e->stream));
    if (ls_old) HIP_TRY(hipMemcpyAsync(ls_old, e->kl_ls_old, (e->pg_shape.two_heads ? tna : (size_t)pg_members(e) * A) * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
