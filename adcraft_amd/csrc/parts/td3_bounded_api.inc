// td3_bounded_api.inc - the extern "C" entry points of the bounded act and of bounded TD3 (include/adcraft_engine.h; the law is
// adc_mlp.h "bounded" and adc_td3.h "bounded"; the kernels are k_mlp_policy's kBounded forms, k_teach_record_bounded and the
// kBounded forms of td3_target_body / td3_actor_body): the deterministic actor squashed into the action box, Gaussian noise
// clipped to the box or a uniform warm-up as its exploration, and a TD3 learner (solo or a population) whose critics read the
// act's action in units of the box.  All of it is opt-in: with the bounds off and the learner unbounded every call launches the
// kernels it launched before.
// (part of the single translation unit adc_engine.hip)
namespace {
// the bounds of the single policy (learners = false) or of the learners: [lo | half | 1 / half] to the device, lo and hi kept on the host
int bounds_set(adc_engine *e, bool learners, const float *lo_a, const float *hi_a)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if ((lo_a == nullptr) != (hi_a == nullptr)) return fail(ADC_EINVAL, "lo and hi: both vectors, or both NULL (bounds off)");
    if (learners) {
        if (e->lrn_M == 0) return fail(ADC_ESTATE, "the learners' bounded act needs learners (adc_engine_mlp_learners)");
    } else {
        if (e->pop_M != 0) return fail(ADC_ESTATE, "the bounded act with a population active is not supported (adc_engine_mlp_population(0) first)");
        if (e->lrn_M != 0) return fail(ADC_ESTATE, "learners are active: their bounds are set through adc_engine_mlp_learners_set_bounds");
    }
    if (lo_a && e->mp.sq_lo)
        return fail(ADC_ESTATE, "the bounded act together with the squashed action is not supported (adc_engine_mlp_set_squash(NULL, NULL) first)");
    if (lo_a && e->mp.two_heads)
        return fail(ADC_ESTATE, "the bounded act needs the policy with the free log_std head: a two-headed policy (2A outputs) is not supported");
    if ((e->have_td3 || e->have_td3_pop) && e->td3_written > 0)
        return fail(ADC_ESTATE, "the replay ring holds transitions: their actions are in units of the bounds as they are, which may not change "
                                "(a new adc_engine_td3_init / adc_engine_td3_pop_init starts an empty ring)");
    const int A = e->mp.A;
    std::vector<float> v((size_t)3 * A);
    for (int a = 0; lo_a && a < A; ++a) {
        if (!std::isfinite(lo_a[a]) || !std::isfinite(hi_a[a]) || !(hi_a[a] > lo_a[a])) return fail(ADC_EINVAL, "action bounds: finite, hi > lo");
        const float half = adc::mlp_squash_half(lo_a[a], hi_a[a]), inv = adc::mlp_inv_half(half);
        if (!std::isfinite(half) || !(half > 0.0f) || !std::isfinite(inv)) return fail(ADC_EINVAL, "action bounds: hi - lo overflows or vanishes");
        v[(size_t)a] = lo_a[a]; v[(size_t)(A + a)] = half; v[(size_t)(2 * A + a)] = inv;
    }
    ENGINE_GUARD(e);
    if (!lo_a) {
        e->mp.bd_lo = e->mp.bd_half = nullptr;
        e->mp.explore = adc::kMlpGaussian;      // (the random mode is the bounded act's alone)
        e->mlp_bd_host.clear();
        return ADC_OK;
    }
    HIP_TRY(hipMemcpyAsync(e->mlp_bd, v.data(), v.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mp.bd_lo = e->mlp_bd; e->mp.bd_half = e->mlp_bd + A;
    e->mlp_bd_host.assign(lo_a, lo_a + A);
    e->mlp_bd_host.insert(e->mlp_bd_host.end(), hi_a, hi_a + A);
    return ADC_OK;
}
// a learner or a population to the bounded law, or back; cfgs: its members' configurations
int td3_bounded_set(adc_engine *e, const adc_td3_config *cfgs, size_t count, int32_t bounded)
{
    if (bounded) {
        if (!e->mp.bd_lo) return fail(ADC_ESTATE, "bounded TD3 needs the bounded act (adc_engine_mlp_set_bounds, or adc_engine_mlp_learners_set_bounds for a population)");
        if (e->td3_norm_set)
            return fail(ADC_ESTATE, "bounded TD3 with an action normalisation is not supported: the critics read the act's action in [-1, 1] as stored");
        for (size_t m = 0; m < count; ++m)
            if (cfgs[m].action_hi > cfgs[m].action_lo)
                return fail(ADC_ESTATE, "bounded TD3 with action_lo / action_hi set is not supported: the target action's box is [-1, 1]");
    }
    if ((bounded != 0) != e->td3_bounded && e->td3_written > 0)
        return fail(ADC_ESTATE, "the replay ring holds transitions: their actions are in the units the learner was stored under, which may not change");
    ENGINE_GUARD(e);
    e->td3_bounded = bounded != 0;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_mlp_set_bounds(adc_engine *e, const float *lo_a, const float *hi_a) { return bounds_set(e, false, lo_a, hi_a); }
ADC_EXPORT int adc_engine_mlp_learners_set_bounds(adc_engine *e, const float *lo_a, const float *hi_a) { return bounds_set(e, true, lo_a, hi_a); }

ADC_EXPORT int adc_engine_mlp_set_explore(adc_engine *e, int32_t mode)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if (mode != ADC_MLP_EXPLORE_GAUSSIAN && mode != ADC_MLP_EXPLORE_RANDOM) return fail(ADC_EINVAL, "unknown exploration mode");
    if (mode == ADC_MLP_EXPLORE_RANDOM && !e->mp.bd_lo)
        return fail(ADC_ESTATE, "the random exploration mode needs the bounded act: actions are drawn uniformly from its box (adc_engine_mlp_set_bounds)");
    ENGINE_GUARD(e);
    e->mp.explore = mode == ADC_MLP_EXPLORE_RANDOM ? adc::kMlpRandom : adc::kMlpGaussian;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_get_bounds(adc_engine *e, float *lo_a, float *hi_a, int32_t *bounded, int32_t *explore)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    const bool on = e->mp.bd_lo != nullptr;
    const size_t A = (size_t)e->mp.A;
    if (on && lo_a) std::copy(e->mlp_bd_host.begin(), e->mlp_bd_host.begin() + (long)A, lo_a);
    if (on && hi_a) std::copy(e->mlp_bd_host.begin() + (long)A, e->mlp_bd_host.end(), hi_a);
    if (bounded) *bounded = on ? 1 : 0;
    if (explore) *explore = e->mp.explore == adc::kMlpRandom ? ADC_MLP_EXPLORE_RANDOM : ADC_MLP_EXPLORE_GAUSSIAN;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_set_bounded(adc_engine *e, int32_t bounded)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return td3_bounded_set(e, &e->td3_cfg, 1, bounded);
}

ADC_EXPORT int adc_engine_td3_pop_set_bounded(adc_engine *e, int32_t bounded)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tp_ready(e)) return rc;
    return td3_bounded_set(e, e->tp_cfg.data(), e->tp_cfg.size(), bounded);
}

ADC_EXPORT int adc_engine_td3_get_bounded(adc_engine *e, int32_t *bounded)
{
    if (!e || !bounded) return fail(ADC_EINVAL, "engine handle or bounded is NULL");
    if (!e->have_td3 && !e->have_td3_pop) return fail(ADC_ESTATE, "adc_engine_td3_init / adc_engine_td3_pop_init has not been called");
    *bounded = e->td3_bounded ? 1 : 0;
    return ADC_OK;
}
