// nstep_api.inc - the extern "C" entry points of n-step returns for the TD3 / SAC trainers, solo or population
// (include/adcraft_engine.h; the law is csrc/adc_td3.h "n-step", the store's window parts/kernel_td3.inc's td3_store_body<.., true>,
// the targets' read of gn td3_target_body / sac_target_body).  The add-on lives in the off-policy trainer's fields: its array
// [M][C] is among td3_allocs and goes with the trainer, the rings' gn point into it.  While it is off (nstep_n == 0) the rings' gn
// are null and every call launches the kernels it launched.  Everything here runs on the engine's own stream behind ENGINE_GUARD.
// (part of the single translation unit adc_engine.hip)
namespace {
inline bool nstep_pop(const adc_engine *e) { return e->have_td3_pop || e->have_sac_pop; }
int nstep_ready(const adc_engine *e)
{
    if (!e->nstep_n) return fail(ADC_ESTATE, "adc_engine_replay_nstep_init has not been called (or its trainer was re-initialised since)");
    return ADC_OK;
}
// member: -1 or 0 for a solo trainer, a population's member otherwise; *m: its row of nstep_gn
int nstep_member(const adc_engine *e, int32_t member, size_t *m)
{
    if (nstep_pop(e) ? (member < 0 || member >= e->lrn_M) : (member != -1 && member != 0)) return fail(ADC_EINVAL, "no such member");
    *m = member < 0 ? 0 : (size_t)member;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_replay_nstep_init(adc_engine *e, int32_t n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (n < 1 || n > adc::kNstepMax) return fail(ADC_EINVAL, "n: 1 to 16 days");
    if (!e->have_td3 && !e->have_sac && !e->have_td3_pop && !e->have_sac_pop)
        return fail(ADC_ESTATE, "n-step returns need a live TD3 or SAC trainer (adc_engine_td3_init / _sac_init / _td3_pop_init / _sac_pop_init)");
    ENGINE_GUARD(e);
    if (!e->nstep_gn) {
        const bool pop = nstep_pop(e);
        const size_t M = pop ? (size_t)e->lrn_M : 1, C = (size_t)e->td3_cfg.capacity;
        // (the array joins the trainer's allocations: what a failure leaves behind goes with it)
        float *gn = nullptr;
        if (int rc = mlp_alloc(e, e->td3_allocs, &gn, M * C)) return rc;
        // what the ring holds is one-step: its slots get their member's gamma (the slots past the size too: a store writes them anew)
        std::vector<float> g0(M * C);
        for (size_t m = 0; m < M; ++m) std::fill(g0.begin() + (ptrdiff_t)(m * C), g0.begin() + (ptrdiff_t)((m + 1) * C), pop ? e->tp_cfg[m].gamma : e->td3_cfg.gamma);
        HIP_TRY(hipMemcpyAsync(gn, g0.data(), M * C * sizeof(float), hipMemcpyHostToDevice, e->stream));
        if (pop) {
            for (size_t m = 0; m < M; ++m) e->tp_mem[m].ring.gn = gn + m * C;
            HIP_TRY(hipMemcpyAsync(e->tp_dmem, e->tp_mem.data(), M * sizeof(Td3Member), hipMemcpyHostToDevice, e->stream));
        } else
            e->td3_ring.gn = gn;
        HIP_TRY(hipStreamSynchronize(e->stream));       // (`g0` is read until here)
        e->nstep_gn = gn;
    }
    e->nstep_n = n;             // (a second init: the window changes from the next store on, the stored slots keep their R and gn)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_nstep_info(adc_engine *e, int32_t *n)
{
    if (!e || !n) return fail(ADC_EINVAL, "engine handle or n is NULL");
    *n = e->nstep_n;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_nstep_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *gn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    size_t m = 0;
    int rc;
    if ((rc = nstep_ready(e)) || (rc = nstep_member(e, member, &m))) return rc;
    if (!gn) return fail(ADC_EINVAL, "gn is NULL");
    if (slot < 0 || count < 1 || slot > td3_size(e) - count) return fail(ADC_EINVAL, "the slot range is not inside [0, size)");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(gn, e->nstep_gn + m * (size_t)e->td3_cfg.capacity + (size_t)slot, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_nstep_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *gn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    size_t m = 0;
    int rc;
    if ((rc = nstep_ready(e)) || (rc = nstep_member(e, member, &m))) return rc;
    if (!gn) return fail(ADC_EINVAL, "gn is NULL");
    if (slot < 0 || count < 1 || slot > (int64_t)e->td3_cfg.capacity - count) return fail(ADC_EINVAL, "the slot range is not inside [0, capacity)");
    const float inf = __builtin_inff();
    for (int64_t i = 0; i < count; ++i)
        if (!(gn[i] >= 0.0f && gn[i] < inf)) return fail(ADC_EINVAL, "a discount must be finite and >= 0");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->nstep_gn + m * (size_t)e->td3_cfg.capacity + (size_t)slot, gn, (size_t)count * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
