// rollout_api.inc - the extern "C" entry points of the rollout record and of the device-resident day loop (include/adcraft_engine.h):
// the record the learned agent's days are written to, and `days` days of any policy in one call.  After the MLP files: a day of
// the learned agent is mlp_day (parts/mlp_core.inc).
// (part of the single translation unit adc_engine.hip)

// ---- the rollout record ----------------------------------------------------------------------------------------------------------------
ADC_EXPORT int adc_engine_rollout_enable(adc_engine *e, int32_t horizon, int32_t fields)
{
    if (int rc = mlp_have(e)) return rc;
    if (horizon < 0 || horizon > (1 << 20)) return fail(ADC_EINVAL, "horizon: 0 (off) to 2^20 days");
    if (fields & ~ADC_ROLLOUT_OBS) return fail(ADC_EINVAL, "unknown rollout field");
    ENGINE_GUARD(e);
    pg_drop(e);                         // (its advantages and scratch were sized for the old record)
    td3_drop(e);
    norm_set_drop(e, e->on);
    mlp_free(e, e->ro_allocs);
    e->ro_T = e->ro_t = 0;
    e->ro_obs = nullptr;
    e->ro_deterministic = false;
    e->ro_teacher = e->ro_dagger = 0;
    e->dg_mask = nullptr;               // (the record's allocation: gone with it)
    if (horizon == 0) return ADC_OK;
    const size_t tn = (size_t)horizon * (size_t)e->v.N;
    int rc;
    if ((rc = mlp_alloc(e, e->ro_allocs, &e->ro_action, tn * (size_t)e->mp.A)) || (rc = mlp_alloc(e, e->ro_allocs, &e->ro_logp, tn)) ||
        (rc = mlp_alloc(e, e->ro_allocs, &e->ro_value, tn)) || (rc = mlp_alloc(e, e->ro_allocs, &e->ro_reward, tn)) ||
        (rc = mlp_alloc(e, e->ro_allocs, &e->ro_term, tn)) || (rc = mlp_alloc(e, e->ro_allocs, &e->ro_trunc, tn)) ||
        ((fields & ADC_ROLLOUT_OBS) && (rc = mlp_alloc(e, e->ro_allocs, &e->ro_obs, tn * (size_t)e->mp.D)))) {
        mlp_free(e, e->ro_allocs);
        e->ro_obs = nullptr;
        return rc;
    }
    e->ro_T = horizon;
    e->ro_fields = fields;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rollout_reset(adc_engine *e)
{
    ENGINE_GUARD(e);
    if (e->ro_T == 0) return fail(ADC_ESTATE, "adc_engine_rollout_enable has not been called");
    e->ro_t = 0;
    for (NormSet *s : {&e->on, &e->rn, &e->tn, &e->sn}) s->t0 = 0;
    e->ro_deterministic = false;
    e->ro_teacher = e->ro_dagger = 0;
    std::fill(e->dg_day.begin(), e->dg_day.end(), (uint8_t)0);
    e->pg_adv_ready = e->im_adv_ready = false;
    e->td3_stored_t = 0;
    e->td3_gap = false;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rollout_fetch(adc_engine *e, int32_t *days_recorded, float *action_tna, float *logp_tn, float *value_tn, float *reward_tn,
                                        uint8_t *terminated_tn, uint8_t *truncated_tn, float *obs_tnd)
{
    ENGINE_GUARD(e);
    if (e->ro_T == 0) return fail(ADC_ESTATE, "adc_engine_rollout_enable has not been called");
    if (obs_tnd && !e->ro_obs) return fail(ADC_ESTATE, "the record was enabled without ADC_ROLLOUT_OBS");
    if (days_recorded) *days_recorded = e->ro_t;
    const size_t tn = (size_t)e->ro_t * (size_t)e->v.N;
    if (tn > 0) {
        if (action_tna) HIP_TRY(hipMemcpyAsync(action_tna, e->ro_action, tn * (size_t)e->mp.A * 4, hipMemcpyDeviceToHost, e->stream));
        if (logp_tn) HIP_TRY(hipMemcpyAsync(logp_tn, e->ro_logp, tn * 4, hipMemcpyDeviceToHost, e->stream));
        if (value_tn) HIP_TRY(hipMemcpyAsync(value_tn, e->ro_value, tn * 4, hipMemcpyDeviceToHost, e->stream));
        if (reward_tn) HIP_TRY(hipMemcpyAsync(reward_tn, e->ro_reward, tn * 4, hipMemcpyDeviceToHost, e->stream));
        if (terminated_tn) HIP_TRY(hipMemcpyAsync(terminated_tn, e->ro_term, tn, hipMemcpyDeviceToHost, e->stream));
        if (truncated_tn) HIP_TRY(hipMemcpyAsync(truncated_tn, e->ro_trunc, tn, hipMemcpyDeviceToHost, e->stream));
        if (obs_tnd) HIP_TRY(hipMemcpyAsync(obs_tnd, e->ro_obs, tn * (size_t)e->mp.D * 4, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// ---- `days` days of the device-resident loop in one call.  Optionally (adc_engine_day_graph_enable) two consecutive
// days (both step parities) are captured once as a hipGraph and replayed.  Measured on MI355X at 1-256 envs x 100
// keywords (tools/measure_small_loop.py): 28-50 us per day either way - the 7 dependent kernels of a day are bound by
// their ~4.5 us each of device-side latency, not by host launch cost - so replay is off by default. ------------------------
namespace {
int one_day(adc_engine *e, int policy, float budget)
{
    int rc = ADC_OK;
    // (the policy kernels and the step are one chain: from the third day on they run group by group where the engine groups at all)
    if (policy == ADC_POLICY_ZERO_MARGIN) {
        if ((rc = agent_step_chained(e, budget))) return rc;
        if (e->have_curves && (rc = ideal_step_chained(e))) return rc;
    } else if (policy == ADC_POLICY_INTERPOLATION) {
        if ((rc = interp_step_chained(e, budget))) return rc;
        if (e->have_curves && (rc = ideal_step_chained(e))) return rc;
    } else if (policy == ADC_POLICY_ORACLE) {
        if ((rc = ideal_step_chained(e))) return rc;
        if ((rc = policy_oracle_chained(e, budget))) return rc;
    } else if (policy == ADC_POLICY_MLP) {
        return mlp_day(e, budget, /* with_ideal = */ true);
    }
    return launch_step(e, e->d_bids, e->d_budget, nullptr, /* lazy_join = */ true);
}
}  // namespace

ADC_EXPORT int adc_engine_day_graph_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    e->day_graph_enabled = enabled != 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_run_days(adc_engine *e, int policy, int32_t days, float budget)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (policy != ADC_POLICY_FIXED_ACTIONS && policy != ADC_POLICY_ZERO_MARGIN && policy != ADC_POLICY_ORACLE &&
        policy != ADC_POLICY_INTERPOLATION && policy != ADC_POLICY_MLP)
        return fail(ADC_EINVAL, "unknown policy");
    if (policy == ADC_POLICY_MLP) {
        if (int ready = mlp_ready(e)) return ready;
        if (days > 0 && !rollout_room(e, days)) return fail(ADC_EINVAL, "the rollout record would overflow within these days: adc_engine_rollout_reset first");
    }
    if (policy == ADC_POLICY_ZERO_MARGIN && !e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    if (policy == ADC_POLICY_INTERPOLATION) {
        if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
        if (days > 0 && !interp_room(e, days)) return fail(ADC_EINVAL, "the interpolation agent's capacity would overflow within these days");
    }
    if (policy == ADC_POLICY_ORACLE && !e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    if (days < 0) return fail(ADC_EINVAL, "days < 0");
    int rc;
    // profiling brackets kernels with events on the stream: keep that path un-captured
    bool use_graph = e->day_graph_enabled && !e->profiling && days >= 4 && policy != ADC_POLICY_MLP;    // (the learned agent's days are never captured)
    if (use_graph && e->v.model == ADC_MODEL_IMPLICIT && e->volume_hint_dirty && !(e->fast_tiles_per_wg && e->fast_variant)) {
        if ((rc = refresh_volume_hint(e))) return rc;        // (synchronises: must not happen inside a capture)
    }
    // (the captured days are one group on the engine's stream; where the plain chain runs as env groups it is the faster of the two -
    //  cfg2: run_days(zero_margin) 0.414 ms per day as one group, 0.247 in groups - so the graph is for engines that do not group)
    if (use_graph && !e->stream_exposed) {
        const adc_engine::StepPlan probe = e->v.model == ADC_MODEL_IMPLICIT ? plan_step(e) : adc_engine::StepPlan{false, false, false};
        if (stream_groups(e, probe, /* chained = */ true) > 1) use_graph = false;
    }
    // The kernel nodes of a captured day hold View and PolicyView BY VALUE (metrics_on, max_days, loss_threshold, drift_*,
    // flat_obs, the curve / grid pointers, n_bids, ...) and the launch shapes derived from the engine's hints: a graph
    // captured under other settings would silently replay them (or read freed curve memory), so the cache key is all of it.
    adc_engine::GraphKey now{};
    std::memset(&now, 0, sizeof(now));              // (padding bytes too: the key is compared with memcmp)
    // (the plan of the captured days is taken HERE, once, and handed to launch_step through capture_plan: the graph and its key
    //  come from the same snapshot of the device's flag words)
    const adc_engine::StepPlan plan = e->v.model == ADC_MODEL_IMPLICIT ? plan_step(e) : adc_engine::StepPlan{false, false, false};
    now.v = e->v; now.pol = e->pol;
    now.have_agent = e->have_agent; now.have_curves = e->have_curves; now.have_ideal = e->have_ideal;
    now.ip = e->ip; now.have_interp = e->have_interp;
    now.mean_volume_hint = e->mean_volume_hint; now.fast_tiles_per_wg = e->fast_tiles_per_wg;
    now.lists = plan.lists;                 // (which variant of the fast pass launch_step picks)
    now.rest = plan.rest;                   // (... and whether k_step_rest_of_day follows the row kernel)
    now.direct = plan.direct;               // (... and its at-once variant)
    if (use_graph && (!e->day_graph || e->day_graph_policy != policy || e->day_graph_budget != budget ||
                      std::memcmp(&now, &e->day_graph_key, sizeof(now)) != 0)) {
        if (e->day_graph) { (void)hipGraphExecDestroy(e->day_graph); e->day_graph = nullptr; }
        if (e->v.model == ADC_MODEL_IMPLICIT && e->v.K <= kRowsMaxK && e->rows_per_cu == 0) {
            // (the occupancy query of launch_step must not run inside a capture: take one plain day first)
            if ((rc = one_day(e, policy, budget))) return rc;
            days -= 1;
        }
        const uint32_t serial0 = e->step_serial;
        const long long stream_steps0 = e->stream_steps;
        const uint64_t env_moves0 = e->env_moves;
        const int last_step0 = e->last_step;
        hipGraph_t graph = nullptr;
        if ((rc = join_groups(e))) return rc;           // (the plain day above may have run as env groups: nothing of it may still be in flight on their streams)
        HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed));
        e->capture_plan = plan;
        e->in_capture = true;
        rc = one_day(e, policy, budget);
        if (!rc) rc = one_day(e, policy, budget);
        e->in_capture = false;
        const hipError_t cap = hipStreamEndCapture(e->stream, &graph);
        e->step_serial = serial0;                       // nothing ran: the capture only recorded the launches
        e->stream_steps = stream_steps0;
        e->last_step = last_step0;
        e->env_moves = env_moves0;
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        HIP_TRY(cap);
        const hipError_t inst = hipGraphInstantiate(&e->day_graph, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        HIP_TRY(inst);
        e->day_graph_policy = policy;
        e->day_graph_budget = budget;
        std::memcpy(&e->day_graph_key, &now, sizeof(now));
        e->day_graph_parity = (int)(serial0 & 1u);
    }
    if (use_graph && days > 0 && (int)(e->step_serial & 1u) != e->day_graph_parity) {
        if ((rc = one_day(e, policy, budget))) return rc;            // line the step parity up with the captured pair
        days -= 1;
    }
    while (use_graph && days >= 2) {
        // (the captured days are one group on the engine's stream: whatever ran as env groups before them is joined first, and what
        //  follows them starts a new chain)
        if ((rc = join_groups(e))) return rc;
        e->last_groups = 1;
        e->needs_fork = e->api_since_step = true;
        if (policy == ADC_POLICY_INTERPOLATION) e->interp_updates += 2;     // (counted before the launch: a failed one errs on the safe side)
        HIP_TRY(hipGraphLaunch(e->day_graph, e->stream));
        e->step_serial += 2;
        e->stream_steps += 2;
        e->env_moves += 2;
        e->last_step = 1;
        e->drift_applied = false;
        days -= 2;
    }
    while (days > 0) {
        if ((rc = one_day(e, policy, budget))) return rc;
        days -= 1;
    }
    return ADC_OK;
}
