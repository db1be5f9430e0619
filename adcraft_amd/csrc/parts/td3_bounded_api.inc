// td3_bounded_api.inc - the extern "C" entry points of bounded TD3 (include/adcraft_engine.h; the law is adc_td3.h "bounded"; the
// kernels are the kBounded forms of td3_target_body / td3_actor_body): a TD3 learner (solo or a population) whose critics read the
// act's action in units of the action box.  The bounded act itself - the bounds, the exploration mode - is parts/mlp_api.inc.  Opt-in:
// with the learner unbounded every call launches the kernels it launched before.
// (part of the single translation unit adc_engine.hip)
namespace {
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
